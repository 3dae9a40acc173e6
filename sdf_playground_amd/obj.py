"""A small Wavefront OBJ writer for the meshes of SDFRenderer.extractMesh: `v`, `vn` and `f` lines with 1-based indices."""


def write_obj(out, positions, normals, indices, comment=None):
    """Writes the mesh to `out` (a path or a text file object): one `v x y z` per vertex, one `vn x y z` per vertex if `normals` is
    given, one `f a//a b//b c//c` (`f a b c` without normals) per triangle.  Floats are written with %.9g, which reads back to the
    same fp32 value.  positions / normals [v, 3], indices [t, 3] (0-based, as extractMesh returns them)."""
    if isinstance(out, (str, bytes)) or hasattr(out, "__fspath__"):
        with open(out, "w") as f:
            return write_obj(f, positions, normals, indices, comment)
    if normals is not None and len(normals) != len(positions):
        raise ValueError("%d normals for %d vertices" % (len(normals), len(positions)))
    if comment:
        for line in str(comment).splitlines():
            out.write("# %s\n" % line)
    for p in positions:
        out.write("v %.9g %.9g %.9g\n" % (float(p[0]), float(p[1]), float(p[2])))
    if normals is not None:
        for n in normals:
            out.write("vn %.9g %.9g %.9g\n" % (float(n[0]), float(n[1]), float(n[2])))
    lines = []
    for t in indices:
        a, b, c = int(t[0]) + 1, int(t[1]) + 1, int(t[2]) + 1
        lines.append("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c) if normals is not None else "f %d %d %d\n" % (a, b, c))
    out.write("".join(lines))
