"""A small Wavefront OBJ writer for the meshes of SDFRenderer.extractMesh: `v`, `vn` and `f` lines with 1-based indices; with the UVs
of a texture atlas (extractMesh(atlas=...)) also `vt` lines, a material library and the atlas as an RGBA8 image."""

MISSING_COLOR = (0.5, 0.5, 0.5)  # a vertex under which no surface was found (surface_colors)


def surface_colors(surfaces):
    """Per-vertex colours [v, 3] float32 of SURFACE_DTYPE records (extractMesh(surfaces=True)): the albedo of a lit material, the
    unlit colour of any other, clipped to [0, 1] (a NaN becomes 0); MISSING_COLOR where valid != 1.  Also returns how many are missing."""
    import numpy as np

    lit = (surfaces["flags"] & 2) != 0  # SDFR_SURFACE_LIT
    rgb = np.where(lit[:, None], surfaces["albedo"], surfaces["unlit"]).astype(np.float32)
    rgb = np.clip(np.nan_to_num(rgb, nan=0.0), 0.0, 1.0)
    missing = surfaces["valid"] != 1
    rgb[missing] = MISSING_COLOR
    return rgb, int(missing.sum())


def openness(occlusion):
    """1 - occluded / 64 of OCCLUSION_DTYPE records as float32 (every value is exact); NaN where valid != 1."""
    import numpy as np

    o = (np.float32(1.0) - occlusion["occluded"].astype(np.float32) / np.float32(64.0)).astype(np.float32)
    o[occlusion["valid"] != 1] = np.nan
    return o


def occlusion_colors(occlusion, colors=None):
    """Per-vertex colours [v, 3] float32 shaded by ambient occlusion: `colors` (surface_colors; without them MISSING_COLOR's grey) times
    the openness of the OCCLUSION_DTYPE records (extractMesh(occlusion=True)); a vertex without an answer keeps its colour."""
    import numpy as np

    o = np.nan_to_num(openness(occlusion), nan=1.0)
    base = np.tile(np.array(MISSING_COLOR, np.float32), (len(o), 1)) if colors is None else np.asarray(colors, np.float32)
    if len(base) != len(o):
        raise ValueError("%d colours for %d occlusion records" % (len(base), len(o)))
    return (base * o[:, None]).astype(np.float32)


def thickness_colors(thickness, t_max):
    """Per-vertex greys [v, 3] float32 of wall thicknesses (SDFRenderer.meshThickness): thickness / t_max clipped to [0, 1]; a vertex
    whose wall does not end within reach (inf) is white, one without a number (NaN) too."""
    import numpy as np

    g = np.clip(np.nan_to_num(np.asarray(thickness, np.float32) / np.float32(t_max), nan=1.0, posinf=1.0), 0.0, 1.0).astype(np.float32)
    return np.repeat(g[:, None], 3, 1)


def lighting_colors(lighting):
    """Per-vertex colours [v, 3] float32 of LIGHTING_DTYPE records (extractMesh(lighting=True)): `lit`, the hit's own colour plus the
    light every unshadowed light delivers, clipped to [0, 1] (a NaN becomes 0); MISSING_COLOR where valid != 1.  Also returns how many
    are missing."""
    import numpy as np

    rgb = np.clip(np.nan_to_num(lighting["lit"].astype(np.float32), nan=0.0), 0.0, 1.0)
    missing = lighting["valid"] != 1
    rgb[missing] = MISSING_COLOR
    return rgb, int(missing.sum())


def atlas_rgba8(plane, valid):
    """An atlas plane [H, W, 3 or 4] float32 (bakeAtlas) as an RGBA8 image [H, W, 4] uint8: rgb clipped to [0, 1] (a NaN becomes 0) as
    surface_colors does, times 255 and rounded; alpha 255.  MISSING_COLOR where valid == 0 (a texel of a quad under which no surface
    was found); alpha 0, and black, where valid == -1 (a texel of no quad)."""
    import numpy as np

    plane, valid = np.asarray(plane, np.float32), np.asarray(valid)
    rgb = np.clip(np.nan_to_num(plane[..., :3], nan=0.0), 0.0, 1.0)
    rgb = np.where((valid == 0)[..., None], np.array(MISSING_COLOR, np.float32), rgb)
    out = np.empty(valid.shape + (4,), np.uint8)
    out[..., :3] = np.floor(rgb * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
    out[..., 3] = 255
    out[valid == -1] = 0
    return out


def write_mtl(path, texture, name="atlas"):
    """Writes a material library with one material `name` whose diffuse map is the image file `texture` (a name relative to the
    library's directory)."""
    with open(path, "w") as f:
        f.write("newmtl %s\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd %s\n" % (name, texture))


def write_obj(out, positions, normals, indices, comment=None, colors=None, uvs=None, material=None, mtllib=None):
    """Writes the mesh to `out` (a path or a text file object): one `v x y z` per vertex -- `v x y z r g b` with `colors` [v, 3], the
    per-vertex colour extension most tools read --, one `vn x y z` per vertex if `normals` is given, one `f a//a b//b c//c`
    (`f a b c` without normals) per triangle.  Floats are written with %.9g, which reads back to the same fp32 value.
    positions / normals [v, 3], indices [t, 3] (0-based, as extractMesh returns them).
    uvs [t, 3, 2] (atlasUVs: origin top-left): one `vt u (1 - v)` per triangle corner -- OBJ's origin is bottom-left; 1 - v is written in full, so that 1 - it reads back to v --, and faces
    `f a/ta/a b/tb/b c/tc/c` (`f a/ta b/tb c/tc` without normals).  material: a `usemtl` line before the faces, and with mtllib (the
    library's file name, write_mtl) a `mtllib` line at the top.  With uvs=None and no material the file is what it always was."""
    if isinstance(out, (str, bytes)) or hasattr(out, "__fspath__"):
        with open(out, "w") as f:
            return write_obj(f, positions, normals, indices, comment, colors, uvs, material, mtllib)
    if uvs is not None and len(uvs) != len(indices):
        raise ValueError("%d triangles of UVs for %d triangles" % (len(uvs), len(indices)))
    if normals is not None and len(normals) != len(positions):
        raise ValueError("%d normals for %d vertices" % (len(normals), len(positions)))
    if colors is not None and len(colors) != len(positions):
        raise ValueError("%d colours for %d vertices" % (len(colors), len(positions)))
    if comment:
        for line in str(comment).splitlines():
            out.write("# %s\n" % line)
    if material and mtllib:
        out.write("mtllib %s\n" % mtllib)
    if colors is not None:
        for p, c in zip(positions, colors):
            out.write("v %.9g %.9g %.9g %.9g %.9g %.9g\n" % (float(p[0]), float(p[1]), float(p[2]), float(c[0]), float(c[1]), float(c[2])))
    else:
        for p in positions:
            out.write("v %.9g %.9g %.9g\n" % (float(p[0]), float(p[1]), float(p[2])))
    if normals is not None:
        for n in normals:
            out.write("vn %.9g %.9g %.9g\n" % (float(n[0]), float(n[1]), float(n[2])))
    if uvs is not None:
        out.write("".join("vt %.9g %r\n" % (float(c[0]), 1.0 - float(c[1])) for tri in uvs for c in tri))
    if material:
        out.write("usemtl %s\n" % material)
    lines = []
    for k, t in enumerate(indices):
        a, b, c = int(t[0]) + 1, int(t[1]) + 1, int(t[2]) + 1
        if uvs is not None:
            ta = 3 * k + 1
            lines.append("f %d/%d/%d %d/%d/%d %d/%d/%d\n" % (a, ta, a, b, ta + 1, b, c, ta + 2, c) if normals is not None
                         else "f %d/%d %d/%d %d/%d\n" % (a, ta, b, ta + 1, c, ta + 2))
            continue
        lines.append("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c) if normals is not None else "f %d %d %d\n" % (a, b, c))
    out.write("".join(lines))
