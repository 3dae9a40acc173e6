"""CPU tier: the scene contract (sdf_playground_amd/csrc/sdfr_scene_traits.h: what a scene may declare, and the default where it does not).
tests/cpp/scene_traits.cpp holds it as static_asserts -- a scene with the mandatory members alone gets every default of the header's table, a
scene that declares everything gets what it declared, inline_escaped_shadows counts only with ray_escapes, and each built-in scene's own
declarations are seen -- so compiling it is the test; the program itself does nothing."""
import os
import subprocess

import cppbuild


def test_the_contract_holds_at_compile_time():
    prog = cppbuild.compile(os.path.join(cppbuild.BUILD, "scene_traits"), [os.path.join(cppbuild.HERE, "cpp", "scene_traits.cpp")],
                            cppbuild.csrc_headers(), cppbuild.EXACT_FLAGS + ["-I" + cppbuild.CSRC], shared=False)
    assert subprocess.run([prog]).returncode == 0
