"""CPU: the ctypes mirror of hgd_unified_batch has the header's size and field offsets, and
hgd_sample_unified / hgd_py_shuffle_rows validate their arguments before touching them."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unified_batch_layout_matches_header(tmp_path):
    from hypergraph_diffusion_for_recommendation_amd import _native
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    py = _native.UnifiedBatch
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hgd.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(hgd_unified_batch));']
    for f, _ in py._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(hgd_unified_batch, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {l.split()[0]: int(l.split()[1]) for l in out if l}
    assert got.pop("size") == ctypes.sizeof(py)
    assert got == {f: getattr(py, f).offset for f, _ in py._fields_}


def test_unified_entry_points_reject_bad_arguments():
    from hypergraph_diffusion_for_recommendation_amd import _native
    lib = _native.load()
    assert lib.hgd_sample_unified(None) == 1                       # HGD_ERR_INVALID_ARG
    mt = np.zeros(625, dtype=np.uint32)
    mt[624] = 625                                                  # a position past the block
    assert lib.hgd_py_shuffle_rows(mt.ctypes.data, None, 10) == 1
    mt[624] = 624
    req = _native.UnifiedBatch()
    req.py_state = req.np_state = mt.ctypes.data
    req.n_items, req.n_sel = 5, 0                                  # an empty selected table
    assert lib.hgd_sample_unified(ctypes.byref(req)) == 1
    assert b"selected-triple table" in lib.hgd_get_last_error_string()
    assert lib.hgd_py_shuffle_rows(mt.ctypes.data, None, 0) == 0   # leaves no error text behind
