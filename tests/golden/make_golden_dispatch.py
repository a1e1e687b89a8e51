#!/usr/bin/env python3
"""Generate tests/golden/arch_dispatch.json: which operators of wave_mamba_amd.ops the arch file calls, in call order, for one
small WaveMamba in four modes (tests/test_arch_dispatch.py compares a later arch file against it).

TEST INFRASTRUCTURE - needs one MI355X and the built library.  The file is a characterisation of ONE commit: record it on the
commit whose dispatch is to be preserved, never on the change under test (`recorded_on` in the file names that commit).  Only
`_OpsBackend.impl` and the public model are used, so the script runs unchanged before and after a rewrite of the arch file.

The model: WaveMamba(in_chn=3, wf=32, n_l_blocks=[1, 1, 1], n_h_blocks=[1, 1, 1], ffn_scale=2) on a (1, 3, 64, 128) image - the
three levels' maps are 32 x 64, 16 x 32 and 8 x 16: levels 1 and 2 take lfss_block_forward's fused closing kernel (W % 32 == 0),
level 3 the unfused pair, and the side streams run.

Usage:  python tests/golden/make_golden_dispatch.py <commit the working tree is at> [output file]
        python tests/golden/make_golden_dispatch.py <commit> --only MODE
The second form re-records ONE mode's line of the committed file - for a change that corrects that mode's dispatch on purpose - and
names the commit in a `MODE_recorded_on` key; every other line stays byte for byte.  (`frozen_input_grad` was re-recorded so with the
fold of CMTAttention.forward asking about its inputs too: the list of 4cb310b recorded attn_fold taken under autograd.)
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "arch_dispatch.json")
MODES = ("eval_two_streams", "eval_one_stream", "train", "frozen_input_grad")
DEV = "cuda:0"


class Recorder:
    """wave_mamba_amd.ops with every operator call noted: attribute lookups go to `ops` (a name it lacks stays an
    AttributeError), the `_supported` predicates come back as they are, any other callable wrapped so that a call appends
    its name to `calls`."""

    def __init__(self, ops):
        self._ops, self.calls = ops, []

    def __getattr__(self, name):
        v = getattr(self._ops, name)
        if not callable(v) or name.endswith("_supported"):
            return v

        def noted(*args, **kwargs):
            self.calls.append(name)
            return v(*args, **kwargs)
        return noted


def run_mode(mode):
    """One forward (and, in the two autograd modes, backward) of the model in `mode`, on whatever backend is installed."""
    import wave_mamba_amd as wm
    torch.manual_seed(0)
    net = wm.WaveMamba(in_chn=3, wf=32, n_l_blocks=[1, 1, 1], n_h_blocks=[1, 1, 1], ffn_scale=2).to(DEV)
    x = torch.rand(1, 3, 64, 128).to(DEV)
    if mode in ("eval_two_streams", "eval_one_stream"):
        net.eval()
        net.restoration_network.two_streams = mode == "eval_two_streams"
        with torch.no_grad():
            net(x)
    else:
        net.train(mode == "train")
        for p in net.parameters():
            p.requires_grad_(mode == "train")
        if mode == "frozen_input_grad":
            x.requires_grad_()
        net(x).sum().backward()
    torch.cuda.synchronize()


def record_only(mode, commit):
    """Replace the line of `mode` in the committed file and set `<mode>_recorded_on`."""
    import wave_mamba_amd as wm
    from wave_mamba_amd.archs import wavemamba_arch as arch
    assert mode in MODES, mode
    rec = Recorder(wm.ops)
    arch._OpsBackend.impl = rec
    try:
        run_mode(mode)
    finally:
        arch._OpsBackend.impl = wm.ops
    with open(OUT) as f:
        lines = [ln.rstrip(",") for ln in f.read().split("\n")[1:-2] if not ln.startswith(json.dumps(mode + "_recorded_on"))]
    at = next(i for i, ln in enumerate(lines) if ln.startswith(json.dumps(mode) + ":"))
    lines[at:at + 1] = [f"{json.dumps(mode)}: {json.dumps(rec.calls)}", f"{json.dumps(mode + '_recorded_on')}: {json.dumps(commit)}"]
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")
    print(f"{mode}: {len(rec.calls)} calls, {len(set(rec.calls))} operators; rewrote that line of {OUT}")


def main():
    import wave_mamba_amd as wm
    from wave_mamba_amd.archs import wavemamba_arch as arch
    if len(sys.argv) == 4 and sys.argv[2] == "--only":
        return record_only(sys.argv[3], sys.argv[1])
    out = {"recorded_on": sys.argv[1]}
    for mode in MODES:
        rec = Recorder(wm.ops)
        arch._OpsBackend.impl = rec
        try:
            run_mode(mode)
        finally:
            arch._OpsBackend.impl = wm.ops
        out[mode] = rec.calls
        print(f"{mode}: {len(rec.calls)} calls, {len(set(rec.calls))} operators")
    path = sys.argv[2] if len(sys.argv) > 2 else OUT
    with open(path, "w") as f:                                 # one line per mode
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in out.items()) + "\n}\n")
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
