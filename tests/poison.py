"""Poisoned scratch memory for tests: a result must not depend on what a buffer held before the call.

A fresh process gets zero pages from the driver, so a kernel that reads a word nobody wrote passes a plain test and fails in a long run, when the
caching allocator hands back a block that held something else.  `poisoned_allocations()` makes that case the normal one: while it is active, whatever
the Python-level allocators return uninitialised -- torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty -- is filled first:

    floating point   NaN
    uint8            0xFF  (a float read through a byte workspace is a NaN too)
    other integers   -1
    bool             True

torch.zeros, torch.full and their kin are untouched.  The fills are ordinary stream-ordered fill_ calls; the originals are restored on exit, also after
an exception.  `poison_(t)` applies the same rule to a buffer the caller passes in (out=, workspace=, loss_out=, a cached module workspace).

The patch is a complete cover of the library's scratch memory because the C side allocates nothing itself: there is no hipMalloc in arlib_amd/csrc
(test_poison_harness_cpu.py greps for it), every workspace and every output is a tensor handed down from Python.

`compare(clean, other)` is the clean-versus-poisoned comparison: it walks two results of the same structure (tensors, numpy arrays, numbers, None,
tuples / lists / dicts of them) and returns the list of places where they are not bit-identical (NaN equals NaN, so a NaN that belongs to the result
does not count as a difference; a NaN that came from the poison does, because the clean run does not have it)."""
import contextlib
import numpy as np
import torch

_FAMILY = ('empty', 'empty_like', 'empty_strided')


def poison_(t):
    """Fill `t` in place by the rule above; returns it.  Tensors without elements and non-tensors pass through."""
    if not isinstance(t, torch.Tensor) or t.numel() == 0:
        return t
    with torch.no_grad():
        if t.is_floating_point() or t.is_complex():
            t.fill_(float('nan'))
        elif t.dtype == torch.uint8:
            t.fill_(0xFF)
        elif t.dtype == torch.bool:
            t.fill_(True)
        else:
            t.fill_(-1)
    return t


def _wrap(fn):
    def poisoned(*args, **kwargs):
        return poison_(fn(*args, **kwargs))
    poisoned.__wrapped__ = fn
    return poisoned


@contextlib.contextmanager
def poisoned_allocations():
    saved = [(torch, name, getattr(torch, name), True) for name in _FAMILY]
    saved.append((torch.Tensor, 'new_empty', torch.Tensor.new_empty, 'new_empty' in vars(torch.Tensor)))      # inherited from the C base class
    try:
        for owner, name, fn, _ in saved:
            setattr(owner, name, _wrap(fn))
        yield
    finally:
        for owner, name, fn, own in saved:
            if own:
                setattr(owner, name, fn)
            else:
                delattr(owner, name)


def _same(a, b):
    if isinstance(a, torch.Tensor):
        if not isinstance(b, torch.Tensor) or a.shape != b.shape or a.dtype != b.dtype:
            return False
        if a.is_floating_point():
            return bool(torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)) and torch.equal(torch.isnan(a), torch.isnan(b)))
        return bool(torch.equal(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'))
    return a == b or (isinstance(a, float) and isinstance(b, float) and a != a and b != b)


def compare(clean, other, path='result'):
    """Places where `other` is not bit-identical to `clean` (empty list = equal)."""
    if isinstance(clean, dict):
        if not isinstance(other, dict) or set(clean) != set(other):
            return [path + ': keys differ']
        return [x for k in clean for x in compare(clean[k], other[k], '%s[%r]' % (path, k))]
    if isinstance(clean, (tuple, list)):
        if not isinstance(other, (tuple, list)) or len(clean) != len(other):
            return [path + ': lengths differ']
        return [x for k in range(len(clean)) for x in compare(clean[k], other[k], '%s[%d]' % (path, k))]
    if _same(clean, other):
        return []
    what = ''
    if isinstance(clean, torch.Tensor) and isinstance(other, torch.Tensor) and clean.shape == other.shape:
        bad = (clean != other) & ~(torch.isnan(clean) & torch.isnan(other)) if clean.is_floating_point() else clean != other
        nan_new = int((torch.isnan(other) & ~torch.isnan(clean)).sum()) if clean.is_floating_point() else 0
        what = ' (%d of %d elements differ, %d of them NaN only in the second)' % (int(bad.sum()), clean.numel(), nan_new)
    return [path + ': not bit-identical' + what]


def has_nan(x):
    """True when any floating-point tensor inside the (nested) result holds a NaN."""
    if isinstance(x, dict):
        return any(has_nan(v) for v in x.values())
    if isinstance(x, (tuple, list)):
        return any(has_nan(v) for v in x)
    return isinstance(x, torch.Tensor) and x.is_floating_point() and x.numel() > 0 and bool(torch.isnan(x).any())
