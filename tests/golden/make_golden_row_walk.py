#!/usr/bin/env python3
"""Generate tests/golden/row_walk_band_rows.json: what wm_lfss_in_conv_band_rows(B, H, W) and wm_lfss_ffn_band_rows(B, H, W) return
over a grid of map sizes (tests/test_row_walk_band_rows.py holds a later library to every value).

TEST INFRASTRUCTURE - host arithmetic only: needs the built library, no GPU.  The file is a characterisation of ONE commit: record
it on the commit whose band heights are to be preserved, never on the change under test (`recorded_on` names that commit).

The grid: B in {1, 2, 8} x H in 1 .. 300 and the UHD heights 544, 1088, 2176 x W in {32, 64, 96, 480, 960, 1920, 3840} - every
width inside both entries' domain (W % 32 == 0, H W <= 2^23).  Values are stored B-major, then H, then W.

Usage:  python tests/golden/make_golden_row_walk.py <commit the working tree is at> [output file]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "row_walk_band_rows.json")
BS = [1, 2, 8]
HS = list(range(1, 301)) + [544, 1088, 2176]
WS = [32, 64, 96, 480, 960, 1920, 3840]


def main():
    from wave_mamba_amd import _lib
    lib = _lib.load()
    out = {"recorded_on": sys.argv[1], "B": BS, "H": HS, "W": WS}
    for key, fn in (("lfss_in_conv", lib.wm_lfss_in_conv_band_rows), ("lfss_ffn", lib.wm_lfss_ffn_band_rows)):
        out[key] = [fn(B, H, W) for B in BS for H in HS for W in WS]
        assert min(out[key]) > 0, key                             # a band height, never a status
    path = sys.argv[2] if len(sys.argv) > 2 else OUT
    with open(path, "w") as f:                                 # one line per key
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in out.items()) + "\n}\n")
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(out['lfss_ffn'])} sizes)")


if __name__ == "__main__":
    main()
