"""The list of query kernel kinds and the kernel lines of a run-time scene's units, as tests/cpp/query_kernels_host.cpp prints them."""
import collections
import os
import subprocess

import cppbuild
import jit_util

Kind = collections.namedtuple("Kind", "index name stem body args size align")
Report = collections.namedtuple("Report", "kinds frame rows query pixel")


def report(scene_text=None):
    """-> Report: QUERY_KERNEL_KINDS, sizeof(FrameU), the rows in the list's order, the kernel lines of the scene's query and pixel units
    (the scene: pendulum.scene.h unless given)"""
    if scene_text is None:
        scene_text = open(os.path.join(jit_util.SCENES_DIR, "pendulum.scene.h")).read()
    exe = cppbuild.plan_program("query_kernels_host")
    out = subprocess.run([exe], input=scene_text, check=True, capture_output=True, text=True).stdout
    kinds = frame = None
    rows, lines = [], {"query": [], "pixel": []}
    for line in out.splitlines():
        what, rest = line.split(" ", 1)
        if what == "kinds":
            kinds = int(rest)
        elif what == "frame":
            frame = int(rest)
        elif what == "kind":
            w = rest.split()
            rows.append(Kind(int(w[0]), w[1], w[2], w[3], w[4], int(w[5]), int(w[6])))
        else:
            lines[what].append(rest)
    return Report(kinds, frame, rows, lines["query"], lines["pixel"])
