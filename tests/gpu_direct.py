"""Helpers of the GPU test files that call the C-ABI directly (tests/test_gpu_conv_f32.py, test_gpu_hgemm_cases.py,
test_gpu_halo_cases.py, test_gpu_thin_cases.py, test_gpu_hsplit_wgrad_cases.py, test_gpu_wgrad_rowring.py): pointers, guarded buffers,
error measures, the operand-range data of the weight-gradient files and the coverage gate that ends a file.  A plain module; the library
is imported inside functions only, as the test files do.  The `_Call` classes stay in their files: each wraps another entry point."""
import ctypes
import functools

import torch

import split_arith

VP = ctypes.c_void_p
GUARD = 4096


def ptr(t):
    return VP(t.data_ptr()) if t is not None else VP(0)


def guarded(dev, nbytes):
    """nbytes of 0xFF with a 0xFF tail behind them"""
    return torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=dev)


def where(t):
    """the index of the largest element"""
    i = int(t.flatten().argmax())
    return tuple(int(v) for v in torch.unravel_index(torch.tensor(i), t.shape))


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def errors(t, ref):
    """(relative L2 error, max |error| of the largest magnitude)"""
    return float((t - ref).norm() / ref.norm()), float((t - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=None)
def range_case(kind, geom, reference):
    """(x, dy, reference(x, dy, geom)) of one operand-range case of a weight gradient on the CPU: made once, shared by the tests that use
    it, never written to.  relu_normal: x after a ReLU, dy = 0.05 randn; wide_range: magnitudes over eight / twelve decades inside one
    tensor; tiny: products near 1e-34 -- normal fp32, but sx sits at the +100 clamp and 1 / (sx sdy) at the edge of the normal range;
    huge: true values near 1e21"""
    N, C, H, W, K, Rr, S, st, pad, pm = geom
    P, Q = split_arith.out_size(H, Rr, st, pad), split_arith.out_size(W, S, st, pad)
    g = torch.Generator().manual_seed(N + C + K + H + W)
    x = torch.randn(N, C, H, W, generator=g)
    dy = torch.randn(N, K, P, Q, generator=g)
    if kind == 'relu_normal':
        x, dy = x.relu_(), dy * 0.05
    else:
        x, dy = split_arith.range_scale(kind, g, x, dy, (8, -6), (12, -14), (1e-30, 1e-4), (1e12, 1e8))
    return x, dy, reference(x, dy, geom)


def coverage_gate(seen, names, instantiations, sections, by_name, inst, line):
    """the body of a file's last test: `seen` maps the names of the cases that ran in this process to (section, instantiation).  Prints
    one COVERAGE line per instantiation (`line` % (instantiation + the cases that ran in each section)); a selection (-k, one worker of
    several) is held to its own cases only, the whole file to every instantiation in every section; a process in which no case ran has
    nothing to check and says so.  Returns whether the whole file ran"""
    assert seen, 'no case of this file ran in this process before this test: nothing was checked (run the whole file in one process)'
    for i in instantiations:
        print(line % (i + tuple(sum(1 for s in seen.values() if s == (sect, i)) for sect in sections)))
    assert {s for s in seen.values()} == {(by_name[n].sect, inst(by_name[n])) for n in seen}
    whole = len(seen) == len(names)
    if whole:
        for sect in sections:
            assert {s[1] for s in seen.values() if s[0] == sect} == set(instantiations), 'section %s: an instantiation no case reached' % sect
    return whole
