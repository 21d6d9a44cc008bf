"""Poisoned scratch memory (tests/poison.py) for the differentiable ALS row solve (arlib_amd/alsgrad.py): the kernels write every output and workspace
word before they read it, so a call on NaN-filled allocations gives the bits of a clean call, and a workspace reused between a large and a small
shape leaves the small shape's results unchanged."""
import inspect

import pytest
import torch
import poison
from test_gpu_poisoned_memory import introspected
from test_gpu_als_poison import SHAPES, inputs

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def grad_inputs(rows, n, d, weighted=True):
    from arlib_amd import alsgrad
    P = inputs(rows, n, d, weighted)
    g = torch.Generator().manual_seed(rows + 3 * d)
    P['gX'] = torch.randn(rows, d, generator=g).to(DEV)                  # non-zero on the empty rows too
    P['Xs'] = {t: alsgrad.als_solve_rows_target(P['Y'], P['G'], P['csr'], P['alpha'], P['reg'], t, route='fused') for t in alsgrad.ALSGRAD_TARGETS}
    return P


def solve_and_backward(m, P, route, s):
    Y = P['Y'].clone().requires_grad_(True)
    csr = P['csr'] if len(P['csr']) == 2 else (P['csr'][0], P['csr'][1], P['csr'][2].clone().requires_grad_(True))
    X = m.als_solve(Y, csr, P['alpha'], P['reg'], 'relaxed', route, split_len=s)
    (X * P['gX']).sum().backward()
    return [X.detach(), Y.grad] + ([csr[2].grad] if len(csr) == 3 else [])


# name -> call(module, problem, split_len); split_len also serves as col_split_len
CASES = {
    'als_solve_rows_target': lambda m, P, s: [m.als_solve_rows_target(P['Y'], P['G'], P['csr'], P['alpha'], P['reg'], t, route='fused', split_len=s)
                                              for t in m.ALSGRAD_TARGETS],
    'als_adjoint_kernel': lambda m, P, s: [m.als_adjoint_kernel(P['Y'], P['G'], P['csr'], P['Xs'][t], P['gX'], P['alpha'], P['reg'], t, split_len=s,
                                                                col_split_len=s, want_dval=w) for t in m.ALSGRAD_TARGETS for w in (True, False)],
    'als_adjoint_composed': lambda m, P, s: m.als_adjoint_composed(P['Y'], P['G'], P['csr'], P['Xs']['relaxed'], P['gX'], P['alpha'], P['reg'], 'relaxed'),
    'als_adjoint': lambda m, P, s: m.als_adjoint(P['Y'], P['G'], P['csr'], P['Xs']['stored'], P['gX'], P['alpha'], P['reg'], 'stored', route='fused',
                                                 split_len=s, col_split_len=s),
    'als_solve': lambda m, P, s: solve_and_backward(m, P, 'fused', s),
}


def test_every_allocating_op_of_the_module_has_a_case():
    from arlib_amd import alsgrad
    found = introspected(inspect.getsource(alsgrad))
    assert {'als_solve_rows_target', 'als_adjoint_kernel'} <= found
    assert sorted(found - set(CASES)) == []
    assert all(hasattr(alsgrad, n) for n in CASES)


@pytest.mark.parametrize('name', sorted(CASES))
@pytest.mark.parametrize('rows,n,d', SHAPES)
@pytest.mark.parametrize('split', [None, 5])
def test_op_is_independent_of_scratch_memory(name, rows, n, d, split):
    from arlib_amd import alsgrad
    for weighted in (False, True):
        P = grad_inputs(rows, n, d, weighted)
        clean = CASES[name](alsgrad, P, split)
        with poison.poisoned_allocations():
            dirty = CASES[name](alsgrad, P, split)
        assert poison.compare(clean, dirty) == []                       # fixed-order reductions: the same bits
        assert not poison.has_nan(dirty)


def test_workspace_reused_between_shapes():
    """The caching allocator hands the second call the first call's blocks (more pieces, wider rows): results equal a fresh process's."""
    from arlib_amd import alsgrad
    big, small = grad_inputs(70, 515, 64), grad_inputs(3, 77, 16)

    def run(P):
        return [CASES[k](alsgrad, P, s) for k in ('als_adjoint_kernel', 'als_solve_rows_target', 'als_solve') for s in (5, None)]
    torch.cuda.empty_cache()
    alone = run(small)
    run(big)
    assert poison.compare(alone, run(small)) == []
