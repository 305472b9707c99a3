"""The tile-GEMM planner with the mixed-height column split (vt_gemm_plan_query3; vitron_amd/csrc/vt_gemm.hip vt_gemm_plan_cost). Host logic
only: the plan queries launch nothing and the library loads without a device.

* gate/up at 5120 rows (C3) runs as 48 column tiles on 320-row tiles (16 x 48 = 768 tiles, three whole rounds of the 256 CUs) + the other 38
  column tiles on 256-row tiles (20 x 38 = 760 tiles, three rounds); at 2560 rows (C3 at 224 px) as 64 column tiles on 320-row tiles (two
  rounds) + 22 on 256-row tiles (one round); at 768 rows (C2 at 224 px) as 64 column tiles on 224-row tiles (one round) + 22 on the 160x128
  ring, with the SwiGLU and the fp32 store: the shapes on which the split was measured faster (profiles/colsplit_gemm_ab.jsonl).
* every other GEMM shape of the C2, C2-224, C3, C3-224, C4 and tower configurations keeps the plan it had: FROZEN is vt_gemm_plan_query2 of
  the commit before the split, and both vt_gemm_plan_query2 (which never reports the new split) and vt_gemm_plan_query3 reproduce it, apart
  from the shapes profiles/colsplit_plans.json lists.
* a split is made of whole column tiles inside the matrix."""
import json
import os

import pytest

from vitron_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W4, W4_320, W4_224 = _lib.CFG_256x256_W4, _lib.CFG_320x256_W4, _lib.CFG_224x256_W4
B, GELU, QGELU, RESID, F32, SWIGLU = (ops.EPI_BF16, ops.EPI_BF16_GELU, ops.EPI_BF16_QGELU, ops.EPI_F32_RESID, ops.EPI_F32, ops.EPI_SWIGLU_BF16)


def config_shapes():
    """(M, N, K, epi) of every GEMM of the decoder (LLaMA-7B: hidden 4096, intermediate 11008) at the prompt lengths of C2 (1088), C2-224 (768),
    C3 (5120), C3-224 (2560) and C4's packed batch (8 x 5120), of the ViT-L/14 towers at their row counts (8 x 577, 577, 8 x 257, 257) and of
    the projector at theirs, with the fp32-output epilogues of the precise modes"""
    out = []
    for S in (1088, 768, 5120, 2560, 40960):
        out += [(S, 12288, 4096, B), (S, 12288, 4096, F32), (S, 8192, 4096, B), (S, 4096, 4096, RESID), (S, 22016, 4096, SWIGLU),
                (S, 22016, 4096, F32), (S, 4096, 11008, RESID)]
    for R in (4616, 577, 2056, 257):
        out += [(R, 3072, 1024, B), (R, 3072, 1024, F32), (R, 1024, 1024, RESID), (R, 4096, 1024, QGELU), (R, 4096, 1024, GELU),
                (R, 4096, 1024, F32), (R, 1024, 4096, RESID)]
    for n in (4608, 576, 2048, 256):
        out += [(n, 4096, 1024, GELU), (n, 4096, 4096, B)]
    return out


# vt_gemm_plan_query2 of the parent commit over config_shapes(), in order: (cfg, rows_first, cols_first)
FROZEN = [
    (16, 0, 0), (16, 0, 0), (16, 0, 0), (15, 0, 0), (16, 0, 0), (16, 0, 0), (15, 0, 0),
    (16, 0, 0), (16, 0, 0), (2, 0, 0), (15, 0, 0), (13, 0, 21760), (13, 0, 21760), (15, 0, 0),
    (14, 0, 0), (14, 0, 0), (14, 0, 0), (14, 0, 0), (13, 0, 0), (13, 0, 0), (14, 0, 0),
    (13, 0, 0), (13, 0, 0), (14, 0, 0), (16, 0, 0), (14, 0, 0), (14, 0, 0), (16, 0, 0),
    (13, 0, 0), (13, 0, 0), (13, 0, 0), (13, 0, 0), (13, 0, 0), (13, 0, 0), (13, 0, 0),
    (16, 0, 0), (16, 0, 0), (15, 0, 0), (14, 0, 0), (14, 0, 0), (14, 0, 0), (15, 0, 0),
    (5, 0, 0), (5, 0, 0), (5, 0, 0), (15, 0, 0), (15, 0, 0), (15, 0, 0), (15, 0, 0),
    (2, 0, 0), (2, 0, 0), (5, 0, 0), (16, 0, 0), (16, 0, 0), (16, 0, 0), (15, 0, 0),
    (5, 0, 0), (5, 0, 0), (5, 0, 0), (5, 0, 0), (5, 0, 0), (5, 0, 0), (15, 0, 0),
    (14, 0, 0), (14, 0, 0), (15, 0, 0), (15, 0, 0), (2, 0, 0), (2, 0, 0), (5, 0, 0),
    (15, 0, 0),
]


def changed_plans():
    with open(os.path.join(ROOT, "profiles", "colsplit_plans.json")) as f:
        return {(p["M"], p["N"], p["K"], p["epi"]): p for p in json.load(f)["changed"]}


def test_gate_up_of_the_headline_fills_whole_rounds():
    assert ops.gemm_plan_split(5120, 22016, 4096, SWIGLU) == (W4_320, 0, 12288, W4)
    assert ops.gemm_plan_split(2560, 22016, 4096, SWIGLU) == (W4_320, 0, 16384, W4)       # measured best of the candidates at 2560 rows
    # the earlier queries cannot name a second configuration: they keep reporting the single grid that ran before
    assert ops.gemm_plan_cols(5120, 22016, 4096, SWIGLU) == (W4, 0, 0) and ops.gemm_plan_cols(2560, 22016, 4096, SWIGLU) == (W4_320, 0, 0)
    # 768 rows: the measured best replaces the same-height split (85 column tiles on 256-row tiles + a 256-column tail), which query2 keeps naming
    for e in (SWIGLU, F32):
        assert ops.gemm_plan_split(768, 22016, 4096, e) == (W4_224, 0, 16384, _lib.CFG_160x128_W4)
        assert ops.gemm_plan_cols(768, 22016, 4096, e) == (W4, 0, 85 * 256)
    # a same-height split is untouched, and query3 names its tail's configuration (768 x 22016 on a loop that was not measured)
    cfg, rows, cols, rest = ops.gemm_plan_split(768, 22016, 2048, SWIGLU)
    assert (cfg, rows, cols) == (W4, 0, 85 * 256) and rest == ops.gemm_plan(768, 22016 - 85 * 256, 2048, SWIGLU)[0]
    # no split: no second configuration
    assert ops.gemm_plan_split(5120, 12288, 4096, B) == (W4_320, 0, 0, _lib.CFG_AUTO)
    assert ops.gemm_plan_split(16, 4096, 4096, B) == (_lib.CFG_SKINNY, 0, 0, _lib.CFG_AUTO)


def test_every_other_shape_keeps_its_plan():
    shapes = config_shapes()
    assert len(shapes) == len(FROZEN)
    changed = changed_plans()
    assert set(changed) == {(5120, 22016, 4096, SWIGLU), (2560, 22016, 4096, SWIGLU), (768, 22016, 4096, SWIGLU), (768, 22016, 4096, F32)}
    seen = 0
    for shape, old in zip(shapes, FROZEN):
        assert ops.gemm_plan_cols(*shape) == old, shape                       # query / query2: unchanged everywhere
        assert ops.gemm_plan(*shape) == old[:2], shape
        new = ops.gemm_plan_split(*shape)
        if shape in changed:
            p = changed[shape]
            assert list(old) == p["old"] and list(new) == p["new"], shape
            seen += 1
        else:
            assert new[:3] == old, shape
    assert seen == len(changed)


def test_splits_are_whole_column_tiles_inside_the_matrix():
    shapes = config_shapes() + [(M, N, K, e) for M in (300, 768, 2560, 5120, 8192 + 512) for N in (4096 + 256, 12288, 22016) for K in (2048, 4096)
                                for e in (B, RESID, SWIGLU)]
    splits = 0
    for M, N, K, e in shapes:
        cfg, rows, cols, rest = ops.gemm_plan_split(M, N, K, e)
        if cols:
            splits += 1
            assert cols % 256 == 0 and 0 < cols < N and rows == 0, (M, N, K, e)
            assert cfg in (W4, W4_320, W4_224) and rest != _lib.CFG_AUTO
            if e == SWIGLU:
                assert cols % 32 == 0                                          # whole [gate 16 | up 16] groups: the output seam is cols / 2
        else:
            assert rest == _lib.CFG_AUTO
    assert splits >= 3


def test_query3_rejects_bad_arguments():
    with pytest.raises(RuntimeError):
        ops.gemm_plan_split(0, 4096, 4096)
