#!/usr/bin/env python3
"""Is the device code of two builds the same, kernel by kernel?  (A move of host code between translation units, a build-script
change, a new compiler flag that should be a no-op: the proof that the GPU runs what it ran before.)

usage: python tools/compare_device_code.py A B       each a gfx950 assembly file (.s) or a directory of them
       python tools/compare_device_code.py A         A against this checkout, compiled now (build.build_variant(asm=True))
       ... --diffs DIR                               also: where the text of a function differs, and which of its loops are untouched

Assembly of this checkout:  python -c "from wave_mamba_amd import build; build.build_variant('build/asm', asm=True)";
of a one-file checkout:     hipcc <build.HIPCC_FLAGS without -shared> -S --cuda-device-only csrc/<file>.hip -o parent.s

Per function symbol: the instruction text (comments, directives and blank lines dropped, local labels renumbered in order of
appearance) and, for kernels, the whole .amdhsa_kernel descriptor (VGPR / SGPR / AGPR counts, scratch and LDS bytes, ...).
Exit status 0 only when both sides hold the same symbols, each once, with identical text and descriptors.

--diffs DIR writes, for every function whose text differs, the unified diff of the normalised text to DIR/<symbol>.diff and prints
the changed line ranges of A and, for every span that a branch jumps back over (label .. last branch back to it: the loops, and the
spans from a label in the prologue to an out-of-line block at the function's end that returns there), its lines and whether B
holds a span of the same text - labels renumbered from the span's own start, so that a label more or fewer in front of it does not
count.  A change confined to the prologue leaves the row loop of a row-walking kernel (its longest proper loop) "identical"."""
import collections
import difflib
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOCAL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def files(path):
    if os.path.isdir(path):
        return sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith(".s"))
    return [path]


def functions(path):
    """-> {symbol: [(normalised instruction text, kernel descriptor or None), ...]}: one list entry per definition"""
    out = collections.defaultdict(list)
    for fn in files(path):
        lines = open(fn).read().split("\n")
        is_function = {m.group(1) for m in (re.match(r"\s*\.type\s+([\w.$]+),@function", ln) for ln in lines) if m}
        desc, cur = {}, None
        for ln in lines:                                          # kernel descriptors
            m = re.match(r"\s*\.amdhsa_kernel\s+([\w.$]+)", ln)
            if m:
                cur = m.group(1); desc[cur] = []
            elif cur and ".end_amdhsa_kernel" in ln:
                cur = None
            elif cur:
                desc[cur].append(" ".join(ln.split()))
        cur, body, labels = None, [], {}
        for ln in lines:
            m = re.match(r"([\w.$]+):", ln)
            if m and m.group(1) in is_function:
                cur, body, labels = m.group(1), [], {}
                continue
            if cur is None:
                continue
            if ln.startswith(".Lfunc_end"):
                out[cur].append(("\n".join(body), "\n".join(desc[cur]) if cur in desc else None))
                cur = None
                continue
            t = ln.split(";")[0].strip()
            if not t or (t.startswith(".") and not LOCAL.match(t)):     # blank / comment-only / directive (labels stay)
                continue
            body.append(LOCAL.sub(lambda mm: labels.setdefault(mm.group(0), f".L{len(labels)}"), " ".join(t.split())))
    return out


def loops(text):
    """[(first line, last line, text with labels renumbered from the span's start)]: every span a branch jumps back over"""
    lines, at, spans = text.split("\n"), {}, {}
    for i, ln in enumerate(lines):
        if ln.endswith(":"):
            at[ln[:-1]] = i
        elif ln.startswith(("s_cbranch", "s_branch")) and ln.split()[-1] in at:
            spans[at[ln.split()[-1]]] = i                         # the last branch back to a label closes its span
    out = []
    for j, i in sorted(spans.items()):
        labels = {}
        out.append((j, i, re.sub(r"\.L\d+", lambda mm: labels.setdefault(mm.group(0), f".L{len(labels)}"), "\n".join(lines[j:i + 1]))))
    return out


def write_diffs(out, fa, fb, names):
    os.makedirs(out, exist_ok=True)
    for s in names:
        ta, tb = fa[s][0][0], fb[s][0][0]
        with open(os.path.join(out, s + ".diff"), "w") as f:
            f.write("\n".join(difflib.unified_diff(ta.split("\n"), tb.split("\n"), "A", "B", n=2, lineterm="")) + "\n")
        ops = difflib.SequenceMatcher(None, ta.split("\n"), tb.split("\n"), autojunk=False).get_opcodes()
        changed = [f"{i1}-{i2}" for tag, i1, i2, _, _ in ops if tag != "equal"]
        print(f"  {s}: {len(ta.split(chr(10)))} / {len(tb.split(chr(10)))} lines, {len(changed)} changed ranges of A: "
              f"{' '.join(changed[:8])}{' ...' if len(changed) > 8 else ''}")
        same = {y[2]: y for y in loops(tb)}
        print("    backward-branch spans of A: " + "; ".join(
            f"{x[0]}-{x[1]} " + (f"identical to B {same[x[2]][0]}-{same[x[2]][1]}" if x[2] in same else "DIFFERS") for x in loops(ta)))


def main():
    diffs = None
    if "--diffs" in sys.argv:
        k = sys.argv.index("--diffs")
        diffs = sys.argv[k + 1]
        del sys.argv[k:k + 2]
    if len(sys.argv) == 2:
        sys.path.insert(0, ROOT)
        from wave_mamba_amd import build
        b = os.path.join(ROOT, "build", "asm")
        build.build_variant(b, asm=True)
    else:
        b = sys.argv[2]
    fa, fb = functions(sys.argv[1]), functions(b)
    dup = [(s, side) for side, f in (("A", fa), ("B", fb)) for s, v in f.items() if len(v) > 1]
    only_a, only_b = sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa))
    text = [s for s in fa if s in fb and fa[s][0][0] != fb[s][0][0]]
    desc = [s for s in fa if s in fb and fa[s][0][1] != fb[s][0][1]]
    nk = sum(1 for v in fb.values() if v[0][1] is not None)
    print(f"A: {len(fa)} device functions in {len(files(sys.argv[1]))} file(s); B: {len(fb)} in {len(files(b))} file(s), {nk} of them kernels")
    print(f"defined more than once: {len(dup)}; only in A: {len(only_a)}; only in B: {len(only_b)}; "
          f"instruction text differs: {len(text)}; kernel descriptor (registers, scratch, LDS) differs: {len(desc)}")
    for what, names in (("twice", dup), ("only in A", only_a), ("only in B", only_b), ("text differs", text), ("descriptor differs", desc)):
        for n in names[:20]:
            print(f"  {what}: {n}")
    if diffs:
        write_diffs(diffs, fa, fb, text)
    return 1 if dup or only_a or only_b or text or desc else 0


if __name__ == "__main__":
    sys.exit(main())
