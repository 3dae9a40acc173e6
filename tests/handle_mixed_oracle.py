"""What the CPU oracle answers for the calls of the mixed sequences (tests/handle_mixed_sequences.py) that came with the survey, the
slices, the spans, the measure, the sharp mesh and the component labelling: each definition of include/sdfr.h as the family's own util module restates it, fed
with the oracle's distances in the step's state.  The CPU tier asks them whether a committed step meets the surface, the GPU tier
compares the reference handle's answers with them.  Test infrastructure: the product never imports this."""
import numpy as np

import components_util
import handle_mixed_sequences as hm
import measure_util
import mesh_sharp_util
import mesh_survey_util
import mesh_util as mu
import query_util as qu
import slice_util
import span_util
import surface_util


def frame(s, w=16, h=9):
    return hm.oracle_frame(qu.po, s["state"], w, h)


def distance(s, of):
    scene = s["state"]["scene"]
    return lambda pts: qu.oracle_points(scene, of, pts, normals=False)[0]


def lattice_distances(s, of, lat=None):
    lat = lat or s["lattice"]
    return distance(s, of)(mu.lattice_points(lat["origin"], lat["cell"], lat["dims"]))


def slices(s, of, stack=None):
    """-> positions, coords, segments, layer_vertices, layer_segments"""
    g = stack or s["slices"]
    D = distance(s, of)(slice_util.lattice_points(g["origin"], g["du"], g["dv"], g["dw"], g["dims"], g["layers"]))
    return slice_util.marching_squares(D, g["origin"], g["du"], g["dv"], g["dw"], g["dims"], g["layers"], 0.0)


def span_rays(s, of, mesh=None, pick=None):
    """(origins, dirs, valid or None) of a span step's items, those of `pick` (indices) if given.  mesh: (positions, normals) of the
    vertices a meshSpans step cycles through"""
    n = s["n"]
    pick = np.arange(n) if pick is None else pick
    if s["call"] == "querySpans":
        o, d = hm.rays(s)
        return np.array(o, np.float32).reshape(-1, 3)[pick], np.array(d, np.float32).reshape(-1, 3)[pick], None
    if s["call"] == "pickSpans":
        px = surface_util.frame_pixels(s["w"], s["h"]) if s["frame"] else np.array(hm.pixel_list(s), np.int32).reshape(-1, 2)
        return span_util.pixel_rays(of, px[pick])
    pos, nrm = mesh
    k = pick % len(pos)
    o, d = span_util.mesh_rays(pos[k], nrm[k], s["reach"])
    return o, d, None


def spans(s, of, rays, max_spans=None):
    """-> (summaries, spans [n, max_spans, 2]) of the rays"""
    min_step, t_max, max_steps = hm.span_params(s)
    p = span_util.params(min_step, t_max, 0.0, max_steps, s["max_spans"] if max_spans is None else max_spans)
    return span_util.march_spans(distance(s, of), rays[0], rays[1], p, rays[2])


def measure_grid(s):
    g = s["grid"]
    return measure_util.grid(g["origin"], g["du"], g["dv"], g["dw"], g["nu"], g["nv"])


def measure(s, of):
    """-> (result dict, columns [nv, nu])"""
    min_step, max_steps = hm.MEASURE_PARAMS[s["march"]]
    return measure_util.measure(distance(s, of), measure_grid(s), span_util.params(min_step, 1.0, s.get("iso", 0.0), max_steps, 0))


def survey(s, of):
    lat = s["lattice"]
    return mesh_survey_util.survey(lattice_distances(s, of), lat["dims"], 0.0, s["band"])


def fit(s, of):
    lat = s["lattice"]
    return mesh_survey_util.fit(mesh_survey_util.oracle_distance(s["state"]["scene"], of), lat["origin"], lat["cell"], lat["dims"], 0.0, s["levels"], s["margin"])


def sharp(s, of):
    """-> the sharp vertices' positions [v, 3]"""
    lat, scene = s["lattice"], s["state"]["scene"]
    f = lambda points, normals: qu.oracle_points(scene, of, points, normals=normals)  # noqa: E731
    return mesh_sharp_util.sharp_nets(lattice_distances(s, of), lat["origin"], lat["cell"], lat["dims"], 0.0, f)[0]


def synthetic_lattice(s):
    """(lattice [pz, py, px], iso) of a labelLattice step: components_util.synthetic of the step's kind, dims and seed"""
    return components_util.synthetic(s["kind"], s["dims"], s["seed"])


def components(s, of=None):
    """-> (counts dict, records, labels [pz, py, px]) by the definition: of the oracle's distances on the step's lattice
    (labelComponents), or of the caller's lattice itself (labelLattice, which needs no frame)"""
    if s["call"] == "labelLattice":
        D, iso = synthetic_lattice(s)
        return components_util.label(D, s["dims"], iso)
    return components_util.label(lattice_distances(s, of), s["lattice"]["dims"], 0.0)


def mesh_vertices(s, of, lat=None):
    """(positions, normals) of the plain extraction over a step's lattice"""
    lat = lat or s["lattice"]
    pos, _idx = mu.surface_nets(lattice_distances(s, of, lat), lat["origin"], lat["cell"], lat["dims"], 0.0)
    return pos, qu.oracle_points(s["state"]["scene"], of, pos)[1]
