"""The inputs of the gradient guard's kernel cases, shared by tests/test_grad_guard_cpu.py (cpu_twin.grad_guard against numpy float64)
and tests/test_grad_guard_gpu.py (the kernel against the twin).  Everything is seeded and built on the CPU; a case is a list of
float32 tensors, each a VIEW that starts `offset` floats behind a 16-byte aligned base (views into a flat buffer start anywhere)."""
import numpy as np
import torch

from wave_mamba_amd import ops

CHUNK = ops.GRAD_GUARD_CHUNK
LENGTHS = [1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 0]
OFFSETS = [0, 1, 2, 3]
MANY = 591
MANY_SIZES = [1 + (i * 4098) // (MANY - 1) for i in range(MANY)]            # 1 ... 4099: both sides of CHUNK
# a tensor whose rows all start one float behind a 16-byte boundary (3 head floats, a 1-float tail; the last row: 3 + 0 + 3);
# "body" lies in the middle of the second row: it is read by a 16-byte load, every other place by a scalar head / tail load
POISON_LEN, POISON_OFFSET = 3 * CHUNK + 6, 1
POISON_PLACES = {"first": 0, "last": POISON_LEN - 1, "head": 1, "tail": CHUNK - 1, "chunk_first": CHUNK, "chunk_last": 2 * CHUNK - 1,
                 "body": CHUNK + 100}
NONFINITE = {"+inf": 0x7f800000, "-inf": 0xff800000, "nan": 0x7fc00000, "nan_payload": 0x7fc00001, "snan": 0x7fa00000}


def at_offset(values, offset, device="cpu"):
    """`values` (1-D float32, CPU) copied bit for bit into a view that starts `offset` floats behind a 16-byte aligned base."""
    n = values.numel()
    buf = torch.zeros(n + offset + 4, dtype=torch.float32, device=device)
    skew = (buf.data_ptr() % 16) // 4                       # (the CPU allocator aligns to 64 bytes, the device's to 256: 0)
    start = (4 - skew) % 4 + offset
    view = buf[start:start + n]
    assert (buf.data_ptr() + 4 * start) % 16 == 4 * (offset % 4) and view.is_contiguous()
    assert n == 0 or view.data_ptr() == buf.data_ptr() + 4 * start
    view.view(torch.int32).copy_(values.view(torch.int32))
    return view


def randn(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


def many(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in MANY_SIZES]


def value_cases():
    """name -> (tensors, finite elements?, norm finite in fp32?)"""
    odd = randn(CHUNK + 5, 3)
    odd[7], odd[CHUNK + 1] = 1e-45, -0.0                    # a denormal and a negative zero are finite
    return {
        "randn": ([randn(2 * CHUNK + 3, 1)], True, True),
        "x1e19": ([randn(2 * CHUNK + 3, 1, 1e19)], True, True),        # squares overflow fp32, the norm does not
        "x1e-30": ([randn(2 * CHUNK + 3, 1, 1e-30)], True, True),      # squares vanish in fp32
        "denormal_negzero": ([odd], True, True),
        "all_3e38": ([torch.full((CHUNK,), 3e38)], True, False),       # finite elements, the norm overflows fp32
    }


def poisoned(bits, place):
    t = randn(POISON_LEN, 5)
    t.view(torch.int32)[POISON_PLACES[place]] = np.array(bits, dtype=np.uint32).astype(np.int32).item()
    return t


def bits_scalar(bits):
    return torch.tensor([np.array(bits, dtype=np.uint32).astype(np.int32).item()], dtype=torch.int32).view(torch.float32)


def numpy_record(tensors, max_norm=None):
    """{norm, found_inf, grad_scale} in numpy: float64 sum of squares, float32 norm and divisor."""
    with np.errstate(all="ignore"):
        arrs = [t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.float32).astype(np.float64) for t in tensors]
        total = np.float64(sum(float(np.sum(a * a)) for a in arrs))
        norm = np.float32(np.sqrt(total))
        found = (not all(np.isfinite(a).all() for a in arrs)) or not np.isfinite(norm)
        scale = np.float32(1.0)
        if max_norm is not None and not found:
            scale = max(np.float32(1.0), (norm + np.float32(1e-6)) / np.float32(max_norm))
    return norm, 1.0 if found else 0.0, np.float32(scale)


def expected_scale(norm, found_inf, max_norm):
    """grad_scale from a record's OWN fp32 norm: max(1, (norm + 1e-6) / max_norm) in fp32, 1 without a max_norm or with found_inf."""
    if max_norm is None or found_inf:
        return np.float32(1.0)
    return max(np.float32(1.0), (np.float32(norm) + np.float32(1e-6)) / np.float32(max_norm))


def norm_within_2ulp(got, want):
    got, want = np.float32(got), np.float32(want)
    return abs(np.float64(got) - np.float64(want)) <= 2.0 * np.float64(np.spacing(np.abs(want)))
