"""The carry launch of the fused SS2D core forward (wm_ss2d_core_fwd): chunk summaries that store sum(dt) instead of P.

The chunk-reduce launch leaves one sum of dt per (chunk, batch, channel) and ss2d_core_carry_kernel forms P = exp2(sum_dt * A) from
it (wm_ss2d_core_carry_select(0), the default); select(1) keeps the earlier form, P stored NP times over and selscan_carry_kernel.
Both fold, combine and re-walk the same 64 segments in the same order, so the carried-in states - and with them every output - have
the same bits.  The shapes are the smallest that reach each regime of the carry kernel (`per` = chunk entries per segment of the
longer pair of directions: a thread keeps its summaries in registers in forms of 16, 24 and 36, above that it streams them
twice); the test prints the chunk counts it ran at."""
import contextlib
import ctypes
import functools

import pytest
import torch

from conftest import assert_close
from oracle import oracle
import wave_mamba_amd as wm
from wave_mamba_amd import _lib
from test_gpu_parity import TOL, cu, random_core_case

gpu = pytest.mark.gpu

#         B  D   H   W     N   R
CASES = [(1, 64, 48, 40, 16, 2),        # several row chunks and column segments; W % 16 != 0; ragged last tiles
         (2, 48, 33, 50, 16, 2),        # channel guard (D < 64), batch 2, odd H
         (1, 64, 32, 1100, 16, 2),      # more than 1024 column chunk entries: per > 16 (the 24-deep register form)
         (1, 64, 40, 72, 24, 3),        # NP = 32, dt_rank 3 (RHI)
         (1, 64, 16, 1700, 16, 2),      # per in 25..36: the 36-deep register form (UHD levels 1 and 2 run it)
         (1, 64, 16, 2400, 16, 2)]      # more than 36 x 64 column chunk entries: summaries streamed twice
PER = {CASES[2]: (17, 24), CASES[4]: (25, 36), CASES[5]: (37, 10 ** 9)}      # the regime a shape is here for (others: <= 16)
BF16_CASE = CASES[0]


@contextlib.contextmanager
def carry_select(mode):
    lib = _lib.load()
    assert lib.wm_ss2d_core_carry_select(mode) == 0
    try:
        yield
    finally:
        assert lib.wm_ss2d_core_carry_select(0) == 0


def chunk_counts(B, D, H, W, N, R):
    """(row_nchunks, col_nchunks, per of the row directions, per of the column directions) from the host's plan."""
    out = (ctypes.c_int * 10)()
    assert _lib.load().wm_ss2d_core_plan(B, D, H, W, N, R, out) == 0
    row, col = out[6], W * out[2]
    return row, col, -(-row // 64), -(-col // 64)


@functools.lru_cache(maxsize=None)
def case_and_oracle(case):
    """The case's operands (CPU) and the CPU oracle's four planes, computed once per shape and never written to."""
    B, D, H, W, N, R = case
    ops = random_core_case(B, D, H, W, N, R, seed=7 * H + W)
    return ops, oracle.ss2d_core_raw(*ops)


def run_both_forms(dev_ops):
    with carry_select(1):
        old4, oldm = wm.ops.ss2d_core(*dev_ops), wm.ops.ss2d_core(*dev_ops, merged=True)
    new4, newm = wm.ops.ss2d_core(*dev_ops), wm.ops.ss2d_core(*dev_ops, merged=True)
    again4, againm = wm.ops.ss2d_core(*dev_ops), wm.ops.ss2d_core(*dev_ops, merged=True)
    return (old4, oldm), (new4, newm), (again4, againm)


def assert_same_bits(a, b, what):
    (a4, am), (b4, bm) = a, b
    for k in range(4):
        assert torch.equal(a4[k], b4[k]), f"{what}: y{k} differs"
    assert torch.equal(am, bm), f"{what}: merged output differs"


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_sum_dt_carry_same_bits_as_stored_p_and_oracle(case):
    row, col, per_row, per_col = chunk_counts(*case)
    print(f"\n{case}: row_nchunks {row}, col_nchunks {col}, per {per_row} (rows) / {per_col} (columns)")
    lo, hi = PER.get(case, (1, 16))
    assert lo <= max(per_row, per_col) <= hi, "the shape no longer reaches the regime it is here for"
    assert row > 64 or col > 64, "more chunk entries than segments in some direction: a segment folds several"
    ops, want = case_and_oracle(case)
    old, new, again = run_both_forms(cu(*ops))
    assert_same_bits(old, new, "stored-P carry against sum_dt carry")
    assert_same_bits(new, again, "two runs of the sum_dt carry")
    for k in range(4):
        assert_close(new[0][k], want[k], TOL, f"core y{k} against the oracle")
    assert_close(new[1], sum(want), TOL, "merged against the oracle")


@gpu
def test_sum_dt_carry_bf16_planes():
    """bf16 planes in and out: the two carry forms agree bit for bit, and the bf16 planes are the fp32 core's output on the same
    (bf16-representable) x rounded once - the fp32 run is held to the oracle at TOL here, so the bf16 one is the oracle's result to
    TOL plus that one rounding (tests/test_gpu_parity.py::test_ss2d_core_bf16_planes states the same property)."""
    B, D, H, W, N, R = BF16_CASE
    ops = list(random_core_case(B, D, H, W, N, R, seed=7 * H + W))
    ops[0] = ops[0].bfloat16().float()
    want = oracle.ss2d_core_raw(*ops)
    dev = cu(*ops)
    old, new, again = run_both_forms([dev[0].bfloat16()] + dev[1:])
    assert all(t.dtype == torch.bfloat16 for t in new[0]) and new[1].dtype == torch.bfloat16
    assert_same_bits(old, new, "bf16 planes, stored-P carry against sum_dt carry")
    assert_same_bits(new, again, "bf16 planes, two runs of the sum_dt carry")
    f32 = wm.ops.ss2d_core(*dev)
    for k in range(4):
        assert_close(f32[k], want[k], TOL, f"fp32 core y{k} against the oracle")
        assert torch.equal(new[0][k], f32[k].bfloat16()), f"y{k}: bf16 core differs from the rounded fp32 core"


def test_selector_and_workspace_bytes_follow_the_plan():
    """Host arithmetic only.  Workspace of the un-merged call = four H arrays [chunks][B D][NP] + four sum_dt arrays [chunks][B D]
    (+ the prep buffer the call fills when it is given none), each rounded up to 256 bytes, with `chunks` the larger of the plan's
    row and column chunk counts; the stored-P form keeps four more H-sized arrays in place of the sum_dt ones."""
    lib = _lib.load()
    assert lib.wm_ss2d_core_carry_select(2) == _lib.WM_EINVAL and lib.wm_ss2d_core_carry_select(-1) == _lib.WM_EINVAL
    B, D, H, W, N, R = CASES[0]
    NP = 16
    row, col, _, _ = chunk_counts(B, D, H, W, N, R)
    chunks = max(row, col)
    up = lambda v: (v + 255) // 256 * 256
    h_bytes, sdt_bytes, prep = up(chunks * B * D * NP * 4), up(chunks * B * D * 4), up(lib.wm_ss2d_core_prep_bytes(N))
    assert sdt_bytes < h_bytes
    assert lib.wm_ss2d_core_fwd_workspace_bytes(B, D, H, W, N, R, 0) == 4 * h_bytes + 4 * sdt_bytes + prep
    plane = up(B * D * H * W * 4)
    assert lib.wm_ss2d_core_fwd_workspace_bytes(B, D, H, W, N, R, 1) == 4 * h_bytes + 4 * sdt_bytes + prep + 3 * plane
    with carry_select(1):
        assert lib.wm_ss2d_core_fwd_workspace_bytes(B, D, H, W, N, R, 0) == 8 * h_bytes + prep
    assert lib.wm_ss2d_core_fwd_workspace_bytes(B, D, H, W, N, R, 0) == 4 * h_bytes + 4 * sdt_bytes + prep
