"""Contours as an SVG file: what SDFRenderer.extractSlices and chainContours return, written as paths.  No dependencies.

One <g> per layer, one <path> per chain.  A point is its lattice coordinates times the cell size; v points up, so
y = (nv - v) * cell: the picture shows the plane as its (u, v) axes draw it.  A closed chain ends in Z; the paths carry
fill-rule="evenodd", so a viewer that fills them leaves holes empty whichever way a loop runs.
"""


def _number(x):
    text = "%.6f" % x
    text = text.rstrip("0").rstrip(".")
    return "0" if text in ("", "-0") else text


def path_data(coords, chain, closed, cell, nv):
    """the `d` attribute of one chain: coords [v][2] lattice coordinates, chain: vertex indices"""
    points = ["%s %s" % (_number(float(coords[k][0]) * cell), _number((nv - float(coords[k][1])) * cell)) for k in chain]
    if not points:
        return ""
    return "M " + " L ".join(points) + (" Z" if closed else "")


def svg_text(coords, layers, dims, cell, stroke_width=None, title=None):
    """The document.  coords: [v][2] lattice coordinates (extractSlices); layers: chainContours' list, one list of (indices, closed) per
    layer; dims = (nu, nv) cells per layer; cell: the size of a lattice cell in the file's units."""
    nu, nv = int(dims[0]), int(dims[1])
    cell = float(cell)
    if not cell > 0 or nu < 1 or nv < 1:
        raise ValueError("svg: dims >= 1 and cell > 0 are needed")
    width, height = nu * cell, nv * cell
    stroke = _number(stroke_width if stroke_width is not None else 0.1 * cell)
    out = ['<?xml version="1.0" encoding="UTF-8"?>',
           '<svg xmlns="http://www.w3.org/2000/svg" version="1.1" width="%s" height="%s" viewBox="0 0 %s %s">'
           % (_number(width), _number(height), _number(width), _number(height))]
    if title:
        out.append("<title>%s</title>" % str(title).replace("&", "&amp;").replace("<", "&lt;").replace(">", "&gt;"))
    for l, chains in enumerate(layers):
        out.append('<g id="layer%d" fill="none" stroke="black" stroke-width="%s" fill-rule="evenodd">' % (l, stroke))
        for chain, closed in chains:
            out.append('<path d="%s"/>' % path_data(coords, chain, closed, cell, nv))
        out.append("</g>")
    out.append("</svg>")
    return "\n".join(out) + "\n"


def write_svg(path, coords, layers, dims, cell, stroke_width=None, title=None):
    with open(path, "w") as fh:
        fh.write(svg_text(coords, layers, dims, cell, stroke_width, title))
