"""Poisoned scratch memory (tests/poison.py) for the ALS ops: the kernels write every output and workspace word before they read it, so a call on
NaN-filled allocations gives the bits of a clean call, and a workspace reused between a large and a small shape leaves the small shape's results
unchanged."""
import inspect

import pytest
import torch
import poison
from test_gpu_poisoned_memory import introspected
from test_als_cpu import problem
from test_gpu_als import on_device

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(3, 77, 16), (70, 515, 64), (33, 300, 128)]


def inputs(rows, n, d, weighted=True):
    from arlib_amd import als
    P = on_device(problem(rows, n, d, 'b', weighted))
    P['G'] = als.gram(P['Y'])
    g = torch.Generator().manual_seed(rows + d)
    P['X'] = (0.1 * torch.randn(rows, d, generator=g)).to(DEV)
    P['sub'] = torch.tensor([rows - 1, 1, 1, 0, 2], dtype=torch.int32, device=DEV)
    return P


# name -> call(module, problem, split_len)
CASES = {
    'gram': lambda als, P, s: als.gram(P['Y']),
    'als_solve_rows_kernel': lambda als, P, s: [als.als_solve_rows_kernel(P['Y'], P['G'], P['csr'], P['alpha'], P['reg'], split_len=s),
                                                als.als_solve_rows_kernel(P['Y'], P['G'], P['csr'], P['alpha'], P['reg'], rows=P['sub'], split_len=s)],
    'als_solve_rows_composed': lambda als, P, s: als.als_solve_rows_composed(P['Y'], P['G'], P['csr'], P['alpha'], P['reg']),
    'als_solve_rows': lambda als, P, s: als.als_solve_rows(P['Y'], P['G'], P['csr'], P['alpha'], P['reg'], route='fused', split_len=s),
    'als_objective': lambda als, P, s: [als.als_objective(P['X'], P['Y'], P['csr'], P['alpha'], P['reg'], G=P['G'], route='fused'),
                                        als.als_objective(P['X'], P['Y'], P['csr'], P['alpha'], P['reg'])],
}


def test_every_allocating_op_of_the_module_has_a_case():
    from arlib_amd import als
    found = introspected(inspect.getsource(als))
    assert {'gram', 'als_solve_rows_kernel', 'als_objective'} <= found
    assert sorted(found - set(CASES)) == []
    assert all(hasattr(als, n) for n in CASES)


@pytest.mark.parametrize('name', sorted(CASES))
@pytest.mark.parametrize('rows,n,d', SHAPES)
@pytest.mark.parametrize('split', [None, 5])
def test_op_is_independent_of_scratch_memory(name, rows, n, d, split):
    from arlib_amd import als
    for weighted in (False, True):
        P = inputs(rows, n, d, weighted)
        clean = CASES[name](als, P, split)
        with poison.poisoned_allocations():
            dirty = CASES[name](als, P, split)
        assert poison.compare(clean, dirty) == []                       # fixed-order reductions: the same bits
        assert not poison.has_nan(dirty)


def test_workspace_reused_between_shapes():
    """The caching allocator hands the second call the first call's blocks (more pieces, wider rows): results equal a fresh process's."""
    from arlib_amd import als
    big, small = inputs(70, 515, 64), inputs(3, 77, 16)

    def run(P):
        return [CASES[k](als, P, s) for k in ('als_solve_rows_kernel', 'als_objective', 'gram') for s in (5, None)]
    torch.cuda.empty_cache()
    alone = run(small)
    run(big)
    assert poison.compare(alone, run(small)) == []
