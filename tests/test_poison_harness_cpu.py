"""The poisoning helper itself (tests/poison.py), on the CPU: the fill rule, what stays untouched, restoration, that a read of one unwritten element
is caught, that the Python patch covers all scratch memory (no allocation on the C side), and one sharded LightGCN step and one sharded PGA step
through the oracle-backed kernel shim under poisoned allocations."""
import os
import re
import sys
import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
from conftest import ROOT
from poison import poisoned_allocations, poison_, compare, has_nan

ORIGINALS = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
FLOATS = (torch.float16, torch.bfloat16, torch.float32, torch.float64)
INTS = (torch.int8, torch.int16, torch.int32, torch.int64)


def patched_now():
    return (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)


def expect_poison(t):
    if t.is_floating_point():
        return bool(torch.isnan(t).all())
    if t.dtype == torch.uint8:
        return bool((t == 0xFF).all())
    if t.dtype == torch.bool:
        return bool(t.all())
    return bool((t == -1).all())


@pytest.mark.parametrize('dtype', FLOATS + INTS + (torch.uint8, torch.bool), ids=str)
def test_fill_rule_per_dtype_and_allocator(dtype):
    like = torch.zeros(5, 3, dtype=dtype)
    with poisoned_allocations():
        made = [torch.empty(7, 3, dtype=dtype), torch.empty((2, 4), dtype=dtype), torch.empty_like(like), torch.empty_strided((3, 4), (4, 1), dtype=dtype),
                like.new_empty(6), like.new_empty((2, 2)), torch.empty(0, dtype=dtype)]
    assert [tuple(t.shape) for t in made] == [(7, 3), (2, 4), (5, 3), (3, 4), (6,), (2, 2), (0,)]
    for t in made:
        assert t.dtype == dtype and expect_poison(t)
    assert expect_poison(poison_(torch.zeros(4, dtype=dtype)))


def test_uint8_workspace_read_as_float_is_nan():
    with poisoned_allocations():
        ws = torch.empty(64, dtype=torch.uint8)
    assert bool(torch.isnan(ws.view(torch.float32)).all()) and bool(torch.isnan(ws.view(torch.float64)).all())
    assert bool((ws.view(torch.int32) == -1).all())                    # and a counter read through it is -1


def test_zeros_family_is_untouched():
    like = torch.ones(3, 2)
    with poisoned_allocations():
        z = [torch.zeros(4), torch.zeros_like(like), like.new_zeros(3), torch.zeros((2, 2), dtype=torch.int32), torch.zeros(3, dtype=torch.uint8)]
        o = [torch.ones(4), torch.ones_like(like), like.new_ones(2)]
        f = [torch.full((3,), 2.5), torch.full_like(like, 2.5), like.new_full((2,), 2.5)]
        a = torch.arange(5)
    assert all(float(t.double().abs().max()) == 0.0 for t in z)
    assert all(bool((t == 1).all()) for t in o) and all(bool((t == 2.5).all()) for t in f)
    assert a.tolist() == [0, 1, 2, 3, 4]


def test_originals_restored_on_exit_and_after_an_exception():
    with poisoned_allocations():
        assert all(a is not b for a, b in zip(patched_now(), ORIGINALS))
    assert all(a is b for a, b in zip(patched_now(), ORIGINALS))
    with pytest.raises(RuntimeError, match='inside'):
        with poisoned_allocations():
            raise RuntimeError('inside')
    assert all(a is b for a, b in zip(patched_now(), ORIGINALS))
    assert 'new_empty' not in vars(torch.Tensor)                       # the method is the C base class's again, not a leftover attribute
    with poisoned_allocations():                                        # nests and unwinds in order
        with poisoned_allocations():
            assert expect_poison(torch.empty(3))
        assert expect_poison(torch.empty(3))
    assert all(a is b for a, b in zip(patched_now(), ORIGINALS))


def planted(x, skip):
    """Sum of x's rows through a scratch buffer whose element `skip` is never written (None: every element is written)."""
    buf = torch.empty(x.shape[0], dtype=x.dtype)
    for r in range(x.shape[0]):
        if r != skip:
            buf[r] = x[r].sum()
    return buf.sum(), buf


@pytest.mark.parametrize('dtype', [torch.float32, torch.int32, torch.uint8], ids=str)
def test_planted_read_before_write_is_reported_as_a_difference(dtype):
    x = (torch.arange(24).reshape(6, 4) % 5).to(dtype)
    clean = planted(x, None)
    with poisoned_allocations():
        good = planted(x, None)
        bad = planted(x, 4)
    assert compare(clean, good) == []
    diff = compare(clean, bad)
    assert len(diff) == 2 and diff[0].startswith('result[0]') and diff[1].startswith('result[1]'), diff
    assert has_nan(bad) == (dtype == torch.float32) and not has_nan(clean)


def test_compare_walks_structures_and_treats_nan_as_equal_to_nan():
    a = {'t': [torch.tensor([1.0, float('nan')]), np.arange(3)], 'n': None, 'f': 2.0}
    b = {'t': [torch.tensor([1.0, float('nan')]), np.arange(3)], 'n': None, 'f': 2.0}
    assert compare(a, b) == []
    b['t'][0] = torch.tensor([float('nan'), float('nan')])
    assert compare(a, b) == ["result['t'][0]: not bit-identical (1 of 2 elements differ, 1 of them NaN only in the second)"]
    assert compare((torch.zeros(2),), (torch.zeros(3),)) and compare([1], [1, 2]) and compare(torch.zeros(2), torch.zeros(2, dtype=torch.int32))
    assert compare(torch.tensor([0.0]), torch.tensor([-0.0])) == []     # value equality: the sign of a zero is not a dependence on scratch memory


def test_c_side_allocates_no_device_memory():
    """The Python patch is a complete cover only while every workspace and output comes from Python: no allocation call in the native sources."""
    csrc = os.path.join(ROOT, 'arlib_amd', 'csrc')
    names = sorted(f for f in os.listdir(csrc) if f.endswith(('.hip', '.cpp', '.h', '.hpp', '.cu')))
    assert 'arl_kernels.hip' in names and 'arl_gan.hip' in names
    pat = re.compile(r'\bhip(Ext)?(Malloc\w*|MemPool\w*|HostAlloc|HostMalloc|MemCreate|MemAddressReserve)\b|\bhsa_\w*memory\w*allocate\b')
    hits = []
    for name in names + ['../../include/arlib_amd.h']:
        with open(os.path.join(csrc, name)) as fh:
            hits += ['%s:%d: %s' % (name, k + 1, line.strip()) for k, line in enumerate(fh) if pat.search(line)]
    assert hits == []


# ---------------------------------------------------------------------------------------------- sharded steps through the CPU shim
def _lightgcn_worker(rank, world, port, ret, poison):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import contextlib
    import torch.distributed as dist
    import cpu_kernels_shim as shim
    from poison import poisoned_allocations as pa
    from test_dist_cpu import small_problem
    from arlib_amd.dist_engine import ShardedPropagationEngine
    os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    U, I, d, L, pairs, E0, batches = small_problem()
    with (pa() if poison else contextlib.nullcontext()):
        eng = ShardedPropagationEngine.from_pairs(pairs, U, I, d, L, 1e-4, 0.005, 'cpu', rank, world, torch.from_numpy(E0.copy()), kernels=shim)
        u, p, n = batches[0]
        lo = eng.step_sparse(torch.from_numpy(u), torch.from_numpy(p), torch.from_numpy(n))
        full = eng.gather_full_table()
        lo = lo.clone()
    if rank == 0:
        ret['table'], ret['loss'] = full.numpy().copy(), lo.numpy().copy()
    dist.destroy_process_group()


def _pga_worker(rank, world, port, ret, poison):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import contextlib
    import torch.distributed as dist
    import cpu_kernels_shim as shim
    from poison import poisoned_allocations as pa
    from test_dist_cpu import pga_problem
    from arlib_amd.dist_engine import ShardedPGA
    os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    U, I, F, L, d, pairs, E0, targets, topk, S0 = pga_problem()
    with (pa() if poison else contextlib.nullcontext()):
        eng = ShardedPGA(pairs, U, F, I, d, L, 'cpu', rank, world, torch.from_numpy(E0.copy()), kernels=shim)
        eng.set_block(S0.copy())
        out, _ = eng.forward()
        top_idx, _ = shim.score_mask_topk(out[:eng.Ul].contiguous(), out[eng.Ul:].contiguous(), topk)
        loss = float(eng.step(targets, top_idx))
    if rank == world - 1:
        ret['S'] = eng.S.numpy().copy()
    if rank == 0:
        ret['loss'] = loss
    dist.destroy_process_group()


def _run(worker, world=2):
    from test_dist_cpu import free_port
    out = []
    for poison in (False, True):
        ret = mp.Manager().dict()
        mp.spawn(worker, args=(world, free_port(), ret, poison), nprocs=world, join=True)
        out.append(dict(ret))
    return out


def test_sharded_lightgcn_step_is_independent_of_scratch_memory():
    clean, poisoned = _run(_lightgcn_worker)
    assert np.isfinite(clean['table']).all() and np.isfinite(clean['loss']).all()
    assert compare(clean, poisoned) == []


def test_sharded_pga_step_is_independent_of_scratch_memory():
    clean, poisoned = _run(_pga_worker)
    assert np.isfinite(clean['S']).all() and np.isfinite(clean['loss'])
    assert compare(clean, poisoned) == []
