"""Build the gfx950 HIP library (and nothing else) in-tree with hipcc.

    python -m wave_mamba_amd.build         # or: python wave_mamba_amd/build.py

Every csrc/*.hip is one translation unit (one kernel family: its launch code, its entry points and the kernel headers it
launches).  The units compile in parallel to objects under build/obj/ (git-ignored) and link into libwavemamba_hip.so, which
sits next to this file (git-ignored too).  An object is rebuilt only when its unit, a header it includes or the flags
changed.  hipcc cross-compiles for gfx950 without a GPU.
"""
import concurrent.futures
import hashlib
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
PUBLIC_HEADER = os.path.join(HERE, "..", "include", "wavemamba_hip.h")
OBJ_ROOT = os.path.join(HERE, "..", "build", "obj")
LIB = os.path.join(HERE, "libwavemamba_hip.so")
ID_UNIT = "common"          # the one unit that sees -DWM_BUILD_ID (wm_build_id): the others do not recompile when the id changes


# -fno-slp-vectorize: the SLP vectoriser pairs independent scalar fp32 operations into packed `v_pk_*_f32` instructions and
# routes halves with op_sel as it likes.  One form it produced - a packed-fp32 op with a SCALAR source and a VGPR source read
# through op_sel = 1 (`v_pk_fma_f32 v, s[..], v, v op_sel:[0,0,1] op_sel_hi:[1,1,0]` in dwconv3x3<bf16>) - returns a zero for the
# re-routed half in lanes 48..63 on MI355X while LDS-fed MFMAs of another kernel share the SIMD: the multi-stream mismatch of
# rounds 4-5 (standalone reproducer tools/ubench_pk_coexec.hip, evidence profiles/r05/).  The packed arithmetic this library
# wants (the scans' state pairs) is written as two-element vectors in the source and is not the vectoriser's work.
# tools/lint_packed_f32.py disassembles the result and refuses a library that contains the form, whoever produced it.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value", "-fno-slp-vectorize"]


def hipcc_path():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: cannot build libwavemamba_hip.so")


def units():
    """Names of the translation units: csrc/<name>.hip."""
    return sorted(f[:-4] for f in os.listdir(CSRC) if f.endswith(".hip"))


def sources():
    """Every file the library is made of: csrc/*.hip, the headers beside them (kernels: *.hip.h) and the public header."""
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))) + [PUBLIC_HEADER]


def source_id(flags=None):
    """sha256 over the compiler flags and the library's sources (sources()), first 16 hex digits: compiled into the library
    (wm_build_id) so that measurements taken on one binary (profiles/pmc_traffic.json) are never quoted for another."""
    h = hashlib.sha256()
    h.update(" ".join(HIPCC_FLAGS if flags is None else flags).encode())    # (a different code generator is a different binary)
    for d in sources():
        with open(d, "rb") as f:
            h.update(os.path.basename(d).encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


def is_stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in sources())


def jobs():
    """Parallel compiles: at most 16, at most MAX_JOBS where set, at most the CPUs there are (never the CPU count alone: a
    shared machine shows hundreds and allows a few)."""
    n = min(16, os.cpu_count() or 1)
    if os.environ.get("MAX_JOBS", "").isdigit():
        n = min(n, int(os.environ["MAX_JOBS"]))
    return max(1, n)


def lint(lib=LIB):
    """_lint_packed_f32.py (same directory) on the built library, EVERY device code object of it (one per unit); raises when the
    vulnerable instruction form is present.  Returns the number of code objects read (None, with a note, where the LLVM binutils
    are absent)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("wave_mamba_amd._lint_packed_f32", os.path.join(HERE, "_lint_packed_f32.py"))
    lint_packed_f32 = importlib.util.module_from_spec(spec)        # (by path: this file also runs as a plain script)
    spec.loader.exec_module(lint_packed_f32)
    if not os.path.exists(os.path.join(lint_packed_f32.LLVM, "llvm-objdump")):
        print("[wave_mamba_amd] llvm-objdump not found: ISA lint skipped", file=sys.stderr)
        return None
    texts = lint_packed_f32.disassemble_all(lib)
    if len(texts) != len(units()):
        raise RuntimeError(f"{lib}: {len(texts)} device code objects for {len(units())} units")
    bad = [b for t in texts for b in lint_packed_f32.offending(t)]
    if bad:
        raise RuntimeError(f"{lib}: {len(bad)} packed-fp32 instruction(s) with unsafe op_sel routing "
                           f"(first: {bad[0][0]}: {bad[0][1]}) - see tools/lint_packed_f32.py")
    return len(texts)


def _dep_paths(dep_file):
    """Prerequisites of a make-style dependency file (-MMD)."""
    with open(dep_file) as f:
        words = f.read().replace("\\\n", " ").split()
    return words[1:]                                             # words[0] is "target:"


def _up_to_date(out, cmd_text):
    """An output is reused when the command that made it is the same, text for text, and nothing it read is newer."""
    try:
        with open(out + ".cmd") as f:
            if f.read() != cmd_text:
                return False
        t = os.path.getmtime(out)
        return all(os.path.getmtime(d) <= t for d in _dep_paths(out + ".d"))
    except OSError:
        return False


def _compile(cmd, out, force):
    cmd_text = " ".join(cmd)
    if not force and _up_to_date(out, cmd_text):
        return None
    if os.path.exists(out + ".cmd"):
        os.remove(out + ".cmd")                                  # (a failed compile leaves no record that matches)
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr)
        raise subprocess.CalledProcessError(r.returncode, cmd)
    with open(out + ".cmd", "w") as f:
        f.write(cmd_text)
    return r.stderr


def build_variant(out, extra_flags=(), drop_flags=(), id_suffix="", only=None, asm=False, check=True, force=False, verbose=False):
    """The one way to compile these sources, for the shipped library (build()) and for every A/B or diagnostics build (tools/).

    out          the shared library to write; with asm=True a directory that receives <unit>.s, the gfx950 assembly
    extra_flags  appended to HIPCC_FLAGS (-D..., -Rpass-analysis=..., ...)
    drop_flags   removed from HIPCC_FLAGS
    id_suffix    appended to wm_build_id() after a "+" (which variant a measurement was taken on)
    only         unit names to compile instead of all (asm=True only: a library needs every unit)
    check        False: link without the ISA lint (a variant built to reproduce what the lint refuses)

    Objects are kept under build/obj/<hash of the flags>/ and reused while their unit, the headers it includes and the command
    line are unchanged, so variants do not evict each other or the release objects.  The library is linked under a temporary
    name, linted (lint()) and moved into place.  Returns {unit: what the compiler wrote to stderr, None where the output was
    reused} - remarks such as -Rpass-analysis=kernel-resource-usage arrive there."""
    flags = [f for f in HIPCC_FLAGS if f not in drop_flags] + list(extra_flags)
    names = units() if only is None else list(only)
    if not asm and names != units():
        raise ValueError("a library is linked from every unit")
    build_id = source_id(flags) + ("+" + id_suffix if id_suffix else "")
    obj_dir = out if asm else os.path.join(OBJ_ROOT, hashlib.sha256(" ".join(flags).encode()).hexdigest()[:12])
    os.makedirs(obj_dir, exist_ok=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    hipcc = hipcc_path()
    unit_flags = [f for f in flags if f != "-shared"]
    cmds = {}
    for u in names:
        o = os.path.join(obj_dir, u + (".s" if asm else ".o"))
        cmds[u] = ([hipcc] + unit_flags + ([f'-DWM_BUILD_ID="{build_id}"'] if u == ID_UNIT else []) +
                   (["-S", "--cuda-device-only"] if asm else ["-c"]) + ["-MMD", "-MF", o + ".d", os.path.join(CSRC, u + ".hip"), "-o", o], o)
    with concurrent.futures.ThreadPoolExecutor(jobs()) as pool:
        futures = {u: pool.submit(_compile, cmd, o, force) for u, (cmd, o) in cmds.items()}
        logs = {u: f.result() for u, f in futures.items()}
    if verbose:
        done = [u for u in names if logs[u] is not None]
        print(f"[wave_mamba_amd] compiled {len(done)} of {len(names)} units ({' '.join(done)}) with {jobs()} jobs: "
              + " ".join(unit_flags), file=sys.stderr)
        sys.stderr.write("".join(v for v in logs.values() if v))
    if not asm:
        subprocess.run([hipcc] + [f for f in flags if f.startswith("--offload-arch")] + ["-shared", "-fPIC"] +
                       [cmds[u][1] for u in names] + ["-o", out + ".tmp"], check=True)
        if check:
            lint(out + ".tmp")
        os.replace(out + ".tmp", out)
    return logs


def build(force=False, verbose=True):
    """Compile csrc/*.hip for gfx950 -> libwavemamba_hip.so (+ the ISA lint).  Returns the path."""
    if not force and not is_stale():
        return LIB
    build_variant(LIB, force=force, verbose=verbose)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
