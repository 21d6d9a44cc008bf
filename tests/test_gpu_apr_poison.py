"""Poisoned scratch memory (tests/poison.py) for APR: the adversarial-BPR op of arlib_amd/advpair.py, util.loss.adv_bpr_loss and engine.step_apr write
every workspace and output word before they read it, so a run on NaN-filled allocations gives the bits of a clean run.  The sweep of
test_gpu_poisoned_memory.py reads arlib_amd/ops.py; this file applies the same introspection to the module the op lives in (the pattern of
test_gpu_pairloss_poison.py)."""
import contextlib
import copy
import inspect
import io

import numpy as np
import pytest
import torch
import poison
import apr_restatement as R
from test_gpu_poisoned_memory import introspected
from test_gpu_apr import _fresh, _batch, dev

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [R.CASES[1], R.CASES[2], R.CASES[3]]          # heavy duplication; across a 256-entry scan trip; across the 512-entry LDS trip


def test_every_allocating_op_of_the_module_has_a_case():
    from arlib_amd import advpair
    assert introspected(inspect.getsource(advpair)) == {'bpr_adv_fwd_bwd'}
    public = {n for n, f in vars(advpair).items() if inspect.isfunction(f) and f.__module__ == advpair.__name__ and not n.startswith('_')}
    assert public == {'bpr_adv_fwd_bwd', 'bpr_adv_supported'}                 # the second is host-only: a shape test, no device memory


def _kernel(case, form, caller_buffers):
    """One call; caller_buffers: workspace, loss_out and delta_out come from the caller and are poisoned by hand."""
    from arlib_amd import ops, _lib
    B, d, U, I, seed = case
    E, u, p, n = R.draw_case(B, d, U, I, seed)
    E = E.astype(np.float32)
    rows = R.batch_rows(u, p, n, U)
    kw = {}
    if caller_buffers:
        kw = {'workspace': poison.poison_(torch.empty(_lib.lib().arl_bpr_adv_workspace_bytes(B, d) // 4 + 5, device=DEV)),
              'loss_out': poison.poison_(torch.empty(2, device=DEV)), 'delta_out': poison.poison_(torch.empty(3 * B, d, device=DEV))}
    if form == 'table':                      # real indices, groups = the row ids, ordered backward into a non-zero G
        G = dev(np.full(E.shape, 0.25, np.float32))
        lo = ops.bpr_adv_fwd_bwd(dev(E), U, dev(u), dev(p), dev(n), 0.5, G=G, upstream=2.0, **kw)
    else:                                    # compact rows, groups given, plain store-add
        ar = torch.arange(B, dtype=torch.int32, device=DEV)
        G = torch.zeros(3 * B, d, device=DEV)
        lo = ops.bpr_adv_fwd_bwd(dev(E[rows]), B, ar, ar, ar + B, 0.5, groups=dev(rows, torch.int32) if form == 'compact' else None, G=G,
                                 distinct_rows=True, **kw)
    return lo, G, kw.get('delta_out')


@pytest.mark.parametrize('form', ['table', 'compact', 'per_position'])
@pytest.mark.parametrize('case', SHAPES, ids=lambda c: 'B%d_d%d' % c[:2])
def test_kernel_is_independent_of_scratch_memory(case, form):
    clean = _kernel(case, form, False)
    with poison.poisoned_allocations():
        alloc = _kernel(case, form, False)
        caller = _kernel(case, form, True)
    assert poison.compare(clean, alloc) == []
    assert poison.compare(clean[:2], caller[:2]) == []
    assert not poison.has_nan(alloc) and not poison.has_nan(caller)            # delta_out included: every row of it is written


@pytest.mark.parametrize('grouped', [True, False])
def test_adv_bpr_loss_is_independent_of_scratch_memory(grouped):
    from arlib_amd.util.loss import adv_bpr_loss
    B, d, U, I, seed = R.CASES[3]
    E, u, p, n = R.draw_case(B, d, U, I, seed)
    rows = R.batch_rows(u, p, n, U)

    def run():
        e = dev(E.astype(np.float32)[rows]).requires_grad_(True)
        loss = adv_bpr_loss(e[:B], e[B:2 * B], e[2 * B:], 0.5, groups=dev(rows) if grouped else None)
        (g,) = torch.autograd.grad(1.5 * loss, e)
        return loss.detach(), g
    clean = run()
    with poison.poisoned_allocations():
        dirty = run()
    assert poison.compare(clean, dirty) == [] and not poison.has_nan(dirty)


@pytest.mark.parametrize('L', [2, 0], ids=['sparse_L2', 'dense_L0'])
def test_step_apr_is_independent_of_scratch_memory(L):
    base = _fresh(apr_encoder='lightgcn' if L else 'mf', n_layers=L)
    u, p, n = _batch(base, B=700)

    def run():
        rec = copy.deepcopy(base)
        eng = rec.model.cuda()._engine(1e-4, 0.005, 'adam')
        eng.reg = 1e-4
        outs = []
        for _ in range(2):                   # the second step reuses the first one's buffers
            lo, adv = eng.step_apr(u, p, n)
            outs.append((lo.clone(), adv.clone()))
        return outs, rec.model._pack().detach().clone()
    clean = run()
    with poison.poisoned_allocations():
        dirty = run()
    assert poison.compare(clean, dirty) == [] and not poison.has_nan(dirty)
