"""CPU tier: SceneLabyrinth::ray_bounds (sdfr_scenes.h; RayBounds, sdfr_scene_traits.h) by a dense walk.  The stand-alone host program
tests/cpp/labyrinth_range_clear.cpp draws 200 000 rays -- starts 4 to 60 high, |dir.y| from 1e-6 to 1, directions up to 6e-4 short of unit
length, ranges from 0.5 to 1000 -- and, wherever the rule sets the flag on a descending ray, walks t from 0 to the range: every sample must be
above 4.01 as ray_escapes sees it, with SceneLabyrinth::dist(..., fast = true) >= 0.002.  It also holds the edge cases: the fma one ulp either
side of 4.01 and on it, dir.y = -0, a NaN in each operand, an infinite range.

Seen with seed 1: 150 000 of the rays descend and the flag fires for 103 698 of them (69 %); no violation.  The control, on a scratch copy of
the headers: the rule with 3.9 in place of 4.01 fails 13 026 walks, the rule with the range halved 5 225, and both fail the edge cases."""
import os
import re
import subprocess

import cppbuild

SRC = os.path.join(cppbuild.HERE, "cpp", "labyrinth_range_clear.cpp")


def test_the_rule_against_a_dense_walk():
    prog = cppbuild.compile(os.path.join(cppbuild.BUILD, "labyrinth_range_clear"), [SRC], cppbuild.csrc_headers(),
                            cppbuild.EXACT_FLAGS + ["-I" + cppbuild.CSRC], shared=False)
    r = subprocess.run([prog, "200000", "1"], capture_output=True, text=True)
    print(r.stdout)
    line = r.stdout.strip().split("\n")[-1]
    got = {k: int(v) for k, v in re.findall(r"(\w+) (-?\d+)", line)}
    assert got["rays"] == 200000 and got["violations"] == 0 and got["edge_violations"] == 0 and got["rising_changed"] == 0, r.stdout
    assert r.returncode == 0, r.stdout + r.stderr
    # the walk is not idle: the flag fires for at least a quarter of the descending rays drawn
    assert got["descending"] >= 100000 and 4 * got["fired"] >= got["descending"], got
