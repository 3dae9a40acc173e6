"""CPU tier of sdfr_mesh_extract: the stage functions of sdfr_mesh.h, built for the host (tests/cpp/mesh_host.cpp) and run sequentially
over a lattice of the oracle's distances, against the definition of include/sdfr.h restated in numpy (mesh_util.surface_nets):
counts, positions bit for bit, indices.  Also the OBJ writer and the command line's box arithmetic."""
import io

import numpy as np
import pytest

import mesh_util as mu
import query_util as qu

# (origin, cell, dims, iso): 40 x 24 x 32 cells of a dyadic edge around the start-up view's content, and a non-dyadic edge with iso != 0
GRIDS = {"dyadic": ((-2.5, -0.25, -2.0), 0.125, (40, 24, 32), 0.0), "cell_0.07": ((-1.4, -0.1, -1.1), 0.07, (40, 24, 32), 0.05)}
SCENES = {"fast_sphere": 0.0, "labyrinth": 1.25, "sierpinski": 0.5}  # scene: time
SHIFT = {"labyrinth": (-3.0, 0.0, -1.5)}  # the start-up view of the labyrinth looks down a corridor: its box moves over a wall's corner


def _grid(scene, name):
    origin, cell, dims, iso = GRIDS[name]
    return tuple(o + s for o, s in zip(origin, SHIFT.get(scene, (0.0, 0.0, 0.0)))), cell, dims, iso


@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_stage_functions_equal_the_definition(scene, grid):
    origin, cell, dims, iso = _grid(scene, grid)
    of = qu.frame(scene, SCENES[scene])
    D, _ = qu.oracle_points(scene, of, mu.lattice_points(origin, cell, dims), normals=False)
    pos_ref, idx_ref = mu.surface_nets(D, origin, cell, dims, iso)
    pos, idx = mu.host_extract(D, origin, cell, dims, iso)
    print("%s %s: %d vertices, %d triangles" % (scene, grid, len(pos_ref), len(idx_ref)))
    assert len(pos_ref) > 100 and len(idx_ref) > 100, "the box misses the scene: the case would show nothing"
    assert pos.shape == pos_ref.shape and idx.shape == idx_ref.shape
    qu.assert_same("%s positions" % scene, pos, pos_ref)
    assert np.array_equal(idx, idx_ref)
    assert idx.max() < len(pos)


def test_definition_on_a_hand_made_lattice():
    # a 2 x 2 x 2 grid whose centre point alone is inside: 8 active cells, 6 edges at the centre, of which only those towards +axis
    # start at the centre; every quad's four cells exist only for the edges that leave the centre point (1, 1, 1) and those that
    # arrive there from (0, 1, 1), (1, 0, 1), (1, 1, 0)
    dims = (2, 2, 2)
    D = np.ones(27, np.float32)
    D[13] = -1.0
    pos, idx = mu.surface_nets(D, (0.0, 0.0, 0.0), 1.0, dims, 0.0)
    hpos, hidx = mu.host_extract(D, (0.0, 0.0, 0.0), 1.0, dims, 0.0)
    assert len(pos) == 8 and len(idx) == 12
    qu.assert_same("positions", hpos, pos)
    assert np.array_equal(hidx, idx)
    # each cell has three crossings, at t = 0.5 on the edges that end in the centre: a closed octahedron-like surface around it
    mu.check_closed_oriented(idx, 8, 2)
    fn, fc = mu.face_normals_and_centroids(pos, idx)
    assert ((fn * (fc - 1.0)).sum(1) > 0).all()  # outward: away from the centre point


def test_nan_is_outside_and_capacity_leaves_arrays_alone():
    dims = (3, 2, 2)
    D = np.linspace(-1.0, 1.0, 4 * 3 * 3, dtype=np.float32)
    D[5] = np.nan
    pos, idx = mu.surface_nets(D, (0.5, 0.0, -1.0), 0.25, dims, 0.0)
    hpos, hidx = mu.host_extract(D, (0.5, 0.0, -1.0), 0.25, dims, 0.0)
    qu.assert_same("positions", hpos, pos)
    assert np.array_equal(hidx, idx)
    # the host program follows the capacity rule of the library: counts only
    import ctypes

    L = mu.host_lib()
    g = mu.HostGrid((ctypes.c_float * 3)(0.5, 0.0, -1.0), 0.25, (ctypes.c_int32 * 3)(*dims), 0.0)
    counts = np.zeros(2, np.int64)
    sentinel = np.full((len(pos), 3), 7.0, np.float32)
    assert L.mh_extract(ctypes.byref(g), qu._p(D), len(pos) - 1, len(idx), qu._p(sentinel), None, qu._p(counts)) == 0
    assert list(counts) == [len(pos), len(idx)] and (sentinel == 7.0).all()


def test_obj_writer_round_trip():
    from sdf_playground_amd.obj import write_obj

    rng = np.random.default_rng(3)
    pos = rng.normal(size=(5, 3)).astype(np.float32)
    nrm = rng.normal(size=(5, 3)).astype(np.float32)
    idx = np.array([[0, 1, 2], [0, 2, 3], [4, 3, 2]], np.uint32)
    text = io.StringIO()
    write_obj(text, pos, nrm, idx, comment="a test")
    v, vn, f = [], [], []
    for line in text.getvalue().splitlines():
        tag, _, rest = line.partition(" ")
        if tag == "v":
            v.append([float(x) for x in rest.split()])
        elif tag == "vn":
            vn.append([float(x) for x in rest.split()])
        elif tag == "f":
            corners = [c.split("/") for c in rest.split()]
            assert all(len(c) == 3 and c[1] == "" and c[0] == c[2] for c in corners)  # a//a
            f.append([int(c[0]) for c in corners])
        else:
            assert tag == "#"
    assert len(v) == 5 and len(vn) == 5 and len(f) == 3
    assert np.array_equal(np.array(v, np.float32), pos) and np.array_equal(np.array(vn, np.float32), nrm)  # %.9g reads back exactly
    assert np.array_equal(np.array(f), idx.astype(np.int64) + 1) and min(min(t) for t in f) == 1  # 1-based
    # without normals: plain `f a b c`
    text = io.StringIO()
    write_obj(text, pos, None, idx)
    assert "vn" not in text.getvalue() and "f 1 2 3\n" in text.getvalue()
    with pytest.raises(ValueError):
        write_obj(io.StringIO(), pos, nrm[:4], idx)


def test_cli_box_arithmetic():
    from sdf_playground_amd import cli

    assert cli.mesh_grid_from_box([-1.0, 0.0, -1.0, 1.0, 1.0, 2.0], 0.25) == ((-1.0, 0.0, -1.0), (8, 4, 12))
    assert cli.mesh_grid_from_box([0.0, 0.0, 0.0, 1.0, 0.05, 0.93], 0.1)[1] == (10, 1, 10)
    for bad in (([0, 0, 0, 1, 1, 1], 0.0), ([0, 0, 0, 0, 1, 1], 0.1), ([0, 0, 0, 2000, 1, 1], 1.0)):
        with pytest.raises(ValueError):
            cli.mesh_grid_from_box(*bad)


@pytest.mark.parametrize("name", sorted(mu.TOPOLOGY))
def test_definition_gives_closed_oriented_surfaces(name):
    # the conditions test_gpu_mesh.py puts to the library, met by the definition itself at these sizes (analytic distances in fp32)
    origin, cell, dims, _euler = mu.TOPOLOGY[name]
    pts = mu.lattice_points(origin, cell, dims)
    D = mu.analytic_distance(name, pts).astype(np.float32)
    assert (D != 0).all()
    pos, idx = mu.surface_nets(D, origin, cell, dims, 0.0)
    hpos, hidx = mu.host_extract(D, origin, cell, dims, 0.0)
    qu.assert_same("positions", hpos, pos)
    assert np.array_equal(hidx, idx)
    mu.check_surface(name, pos, idx, cell, mu.analytic_distance(name, pos), lambda p: mu.analytic_normal(name, p))
