"""CPU: the object stream's normals entry points exist in the header, the library and the ctypes
table, and the Batch(normals=True) convenience leaves the caller's settings alone (no GPU call)."""
import copy
import inspect
import json
import os

from conftest import ROOT
from test_cpu import _header_functions

NEW = ["implisolid_batch_download_normals", "implisolid_batch_has_normals"]


def test_library_exports_the_batch_normals_symbols(impli):
    L = impli.lib()
    declared = _header_functions()
    for name in NEW:
        assert name in declared and name in impli.ABI_SYMBOLS, name
        f = getattr(L, name)
        assert f.argtypes is not None and len(f.argtypes) == (4 if "download" in name else 1), name
    # the header no longer says that the stream ignores the key
    txt = " ".join(open(os.path.join(ROOT, "include", "implisolid.h")).read().split())
    assert "(implisolid_batch_*) ignores the key" not in txt and "an object stream computes no normals" not in txt


def test_with_normals_leaves_the_callers_settings_unchanged(impli):
    from implisolid_amd import scenes
    mc = scenes.mc_settings(24, 1.0)
    for given in (mc, dict(mc, normals={"enabled": 0, "other": 7}), dict(mc, normals=3)):
        before = copy.deepcopy(given)
        out = impli._with_normals(given, True)
        assert given == before and out is not given
        assert out["normals"]["enabled"] == 1 and {k: v for k, v in out.items() if k != "normals"} == \
            {k: v for k, v in before.items() if k != "normals"}
        if isinstance(before.get("normals"), dict):
            assert out["normals"] is not given["normals"] and out["normals"]["other"] == 7
        assert impli._with_normals(given, False) is given
    text = json.dumps(mc)
    assert json.loads(json.dumps(impli._with_normals(text, True)))["normals"] == {"enabled": 1}
    assert impli.parse_settings(impli._with_normals(mc, True))["resolution"] == 24
    # Batch(..., normals=...) goes through it, and download / normals take the new arguments
    assert "_with_normals(mc_settings, normals)" in inspect.getsource(impli.Batch.__init__)
    assert list(inspect.signature(impli.Batch.download).parameters) == ["self", "i", "normals"]
    assert list(inspect.signature(impli.Batch.normals).parameters) == ["self", "i", "return_problems"]
