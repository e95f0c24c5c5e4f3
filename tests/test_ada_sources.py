"""The Ada side (ada/) cannot be compiled in this image: scripts/check_ada_sources.py checks it textually against the
reference's specs instead -- every name used is declared, every `Package.Name` names something that package declares.
That check of ada/ needs a checkout of the reference (`python scripts/check_ada_sources.py <madarch checkout>`), which
the repository does not hold; here the checker and the patch script run on a stand-in checkout written by the tests."""
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Stand-ins for the three files ada/apply_patches.sh edits: the lines it looks for, around them a minimal unit
STAND_INS = {
    "madarch-scenes.ads": "package Madarch.Scenes is\n   type Scene is private;\n   function Compile return Scene;\nprivate\n"
                          "   type Scene_Internal is record\n      GPU_Type : GPU_Types.GPU_Type;\n   end record;\nend Madarch.Scenes;\n",
    "madarch-scenes.adb": "package body Madarch.Scenes is\n   function Compile return Scene is\n   begin\n      return new Scene_Internal'\n"
                          "        (GPU_Type => Compute_Scene_GPU_Type (Kinds),\n         others => <>);\n   end Compile;\nend Madarch.Scenes;\n",
    "madarch-renderers.ads": "package Madarch.Renderers is\n   type Renderer is private;\nprivate\n   type Renderer_Internal is record\n"
                             "      Screen_Pass : Shaders.Program;\n   end record;\nend Madarch.Renderers;\n",
}


def _stand_in_checkout(tmp_path):
    root = tmp_path / "checkout"
    (root / "madarch" / "support").mkdir(parents=True)
    for name, text in STAND_INS.items():
        (root / "madarch" / name).write_text(text)
    return str(root)


def _checker():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import check_ada_sources
    return check_ada_sources


def test_the_checker_sees_a_call_of_a_subprogram_that_does_not_exist(tmp_path):
    """... such as the Scenes.Describe / Scenes.Kind_Index of the first round's body, which Madarch.Scenes never had"""
    ada = tmp_path / "ada"
    shutil.copytree(os.path.join(ROOT, "ada"), ada)
    ref = _stand_in_checkout(tmp_path)
    before = _checker().check(ref, str(ada))  # (the stand-in declares little of what ada/ uses: findings on many lines)
    body = (ada / "madarch-renderers.adb").read_text()
    mutations = {"Scenes.HIP.Describe (Scene, Desc, Keep);": "Scenes.Describe (Scene, Desc);",
                 "Scenes.HIP.Kind_Index (Self.Scene, Lit)": "Scenes.HIP.Index_Of_Kind (Self.Scene, Lit)"}
    mutated = set()
    for old, new in mutations.items():
        assert old in body
        mutated |= {("madarch-renderers.adb", n + 1) for n, line in enumerate(body.splitlines()) if old in line}
        body = body.replace(old, new)
    (ada / "madarch-renderers.adb").write_text(body)
    found = _checker().check(ref, str(ada))
    assert any("`Scenes` declares no `describe`" in f for f in found), found
    assert any("index_of_kind" in f.lower() for f in found), found

    def where(f):
        m = re.search(r"([\w.-]+\.ad[sb]):(\d+):", f)
        return m.group(1), int(m.group(2))
    # every line the mutations did not touch gives what it gave before: the checker is quiet on what did not change
    assert sorted(f for f in found if where(f) not in mutated) == sorted(f for f in before if where(f) not in mutated)


def test_patches_apply_to_the_reference(tmp_path):
    """The script's three edits, on stand-ins holding the lines its patterns look for: whether those patterns match
    the reference's own files is checked only where a checkout is at hand (apply_patches.sh exits 1 otherwise)."""
    out = tmp_path / "out"
    subprocess.check_call(["bash", os.path.join(ROOT, "ada", "apply_patches.sh"), _stand_in_checkout(tmp_path), str(out)])
    assert "Max_Dist : GL.Types.Single" in (out / "madarch-scenes.ads").read_text()
    assert "Max_Dist => Max_Dist," in (out / "madarch-scenes.adb").read_text()
    spec = (out / "madarch-renderers.ads").read_text()
    assert "Handle : System.Address" in spec and "Screen_Pass" not in spec
