"""Level-checkpointed traceback (BIALIGN_BATCH_LEVEL_TRACE), the parts a machine without a GPU can check: the flag in
the header and the binding, the unchanged ABI, and the argument checks that run before any library call."""
import ctypes
import os
import re

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "bialign.h")


def lib_module():
    try:
        from bialign_amd import _lib
    except (ImportError, OSError) as e:  # the library is built by __graft_entry__.build()
        pytest.fail(f"libbialign_hip.so does not load: {e}")
    return _lib


def test_flag_value_in_header_and_binding():
    text = open(HEADER).read()
    m = re.search(r"^#define\s+BIALIGN_BATCH_LEVEL_TRACE\s+(\d+)u\s*$", text, re.M)
    assert m and int(m.group(1)) == 4
    assert lib_module().BATCH_LEVEL_TRACE == 4
    # a bit of its own next to the other two storage flags
    assert lib_module().BATCH_LEVEL_TRACE & (lib_module().BATCH_SCORE_ONLY | lib_module().BATCH_LEAN_TRACE) == 0


def test_abi_and_struct_layouts_unchanged():
    _lib = lib_module()
    assert _lib.BATCH_LEVEL_TRACE == 4
    assert _lib.ABI_VERSION == 10 and _lib.lib.bialign_abi_version() == 10
    assert re.search(r"^#define\s+BIALIGN_ABI_VERSION\s+10\s*$", open(HEADER).read(), re.M)
    assert ctypes.sizeof(_lib.BatchInfo) == 56
    assert ctypes.sizeof(_lib.Timing) == 40
    assert ctypes.sizeof(_lib.Params) == 24


@pytest.mark.parametrize("other", ["score_only", "lean_trace"])
def test_make_batch_rejects_level_trace_with_another_storage_mode(other, monkeypatch):
    """ValueError before the engine is touched: the Batch class is replaced by one that fails the test if reached."""
    from bialign_amd import batch, synth
    lib_module()
    import bialign_amd.engine as engine

    def unreachable(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(engine, "Batch", unreachable)
    monkeypatch.setattr(engine, "default_engine", unreachable)
    pair = synth.protein_pair(1, 12, 13)
    params = dict(synth.PROTEIN_PARAMS, max_shift=6)
    with pytest.raises(ValueError, match="level_trace"):
        batch.make_batch([pair], params, level_trace=True, **{other: True})
    mols = [("ACGUACGU", ([0.2] * 8, [0.3] * 8, [0.5] * 8))]
    with pytest.raises(ValueError, match="level_trace"):
        batch.make_feature_batch(mols, [(0, 0)], dict(synth.RNA_PARAMS, max_shift=6), level_trace=True, **{other: True})
