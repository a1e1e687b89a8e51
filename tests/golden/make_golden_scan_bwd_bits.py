#!/usr/bin/env python3
"""Generate tests/golden/scan_bwd_bits.json: the SHA-256 of the bytes of every gradient of the scan backward, per case of
tests/test_scan_bwd_bits.py (which holds a later library to every hash).

TEST INFRASTRUCTURE - needs an MI355X.  The file is a characterisation of ONE commit: record it with the library of the commit
whose bits are to be preserved (WAVEMAMBA_HIP_LIB=<that commit's libwavemamba_hip.so>, `recorded_on` names the commit), never
with the build under test.  Every case runs twice; the two runs must agree before anything is written.

The two cases whose point is a block of more than one chunk are checked against the plan: the library exposes the plan only as
workspace sizes, so the block lengths are recomputed here by the plan's own rules (scan_bwd.hip: bwd_plan, bwd_fused_cpb), and the
op-boundary one is confirmed through wm_selscan_bwd_workspace_bytes, which depends on the number of blocks.

Usage:  python tests/golden/make_golden_scan_bwd_bits.py <commit of the library in use> [output file]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(HERE, "scan_bwd_bits.json")


def up(v):
    return (v + 255) // 256 * 256


def scan_cpb(batch, dim, L, N, G):
    """bwd_plan: at least 2048 blocks, at most 16 chunks each"""
    rows = batch * G * ((dim // G + 63) // 64)
    nchunks = (L + 15) // 16
    return max(1, min(16, nchunks * rows // 2048)), nchunks


def scan_workspace_bytes(batch, dim, L, N, G, cpb):
    """BwdPlan::total for a given block length (carry segments of 32 blocks)"""
    NP = 16 if N <= 16 else 32
    nchunks = (L + 15) // 16
    nblocks = (nchunks + cpb - 1) // cpb
    chains = batch * dim * NP
    return (4 * up(nblocks * chains * 4) + up(nchunks * chains * 4) + up(nchunks * batch * dim * 4) +
            up(4 * ((nblocks + 31) // 32) * chains * 4) + up(nblocks * batch * dim * (NP + 4) * 4))


def fused_cpb(B, L, N):
    """bwd_fused_cpb: whole dispatch rounds of resident workgroups, ties to the longer block"""
    resident = 1024 if N <= 16 else 512
    nchunks = (L + 15) // 16
    best, best_cost = 1, 1e300
    for c in range(1, 33):
        wgs = (nchunks + c - 1) // c * B
        cost = ((wgs + resident - 1) // resident) * (c + 0.4)
        if cost <= best_cost:
            best, best_cost = c, cost
    return best


def main():
    import test_scan_bwd_bits as t
    from wave_mamba_amd import _lib
    lib = _lib.load()
    big = t.SCAN_CASES[-1]
    cpb, nchunks = scan_cpb(*big)
    assert cpb > 1, (big, cpb)
    got = lib.wm_selscan_bwd_workspace_bytes(*big)
    assert got == scan_workspace_bytes(*big, cpb) != scan_workspace_bytes(*big, 1), (got, cpb)
    B, D, H, W, N, R, _ = t.CORE_CASES[-1]
    assert fused_cpb(B, H * W, N) > 1, t.CORE_CASES[-1]
    assert all(scan_cpb(*c)[0] == 1 for c in t.SCAN_CASES[:-1])
    assert all(fused_cpb(c[0], c[2] * c[3], c[4]) == 1 for c in t.CORE_CASES[:-1])
    cases = {}
    for cid, fn, shape in t.all_cases():
        first, second = fn(*shape), fn(*shape)
        assert first == second, f"{cid}: two runs differ - not a case a hash can judge"
        cases[cid] = first
    out = {"recorded_on": sys.argv[1], "library": _lib.build_id(), "cases": cases}
    path = sys.argv[2] if len(sys.argv) > 2 else OUT
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(cases)} cases, library {out['library']})")


if __name__ == "__main__":
    main()
