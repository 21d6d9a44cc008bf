"""Poisoned scratch memory (tests/poison.py) for GSPAttack: the all-pairs BCE kernel writes every output and workspace word before it reads it,
so a call on NaN-filled allocations gives the bits of a clean call; so does one whole attack epoch."""
import inspect

import pytest
import torch
import poison
from test_gpu_poisoned_memory import introspected
from test_gpu_gsp import problem, on_device, attack_problem, run_device_attack

pytestmark = pytest.mark.gpu

# (R, I, d, positives per row): three splits of the streamed users with a ragged last one, ragged tiles at the narrowest and the widest rows
SHAPES = [(9001, 333, 64, 5), (130, 77, 16, 3), (2049, 515, 128, 4)]
CASES = {
    'bce_allpairs_loss': lambda ap, P, g: ap.bce_allpairs_loss(*P, want_grad=g),
    'bce_allpairs_loss_composed': lambda ap, P, g: ap.bce_allpairs_loss_composed(*P, want_grad=g),
}


def test_every_allocating_op_of_the_module_has_a_case():
    from arlib_amd import allpairs as ap
    found = introspected(inspect.getsource(ap))
    assert 'bce_allpairs_loss' in found                                 # the introspection sees the kernel wrapper's torch.empty
    assert sorted(found - set(CASES)) == []


@pytest.mark.parametrize('name', sorted(CASES))
@pytest.mark.parametrize('R,I,d,per_row', SHAPES)
@pytest.mark.parametrize('grad', [False, True])
def test_op_is_independent_of_scratch_memory(name, R, I, d, per_row, grad):
    from arlib_amd import allpairs as ap
    P = on_device(*problem(R, I, d, per_row, 0.15, seed=R, weighted=True))
    clean = CASES[name](ap, P, grad)
    with poison.poisoned_allocations():
        dirty = CASES[name](ap, P, grad)
    if name == 'bce_allpairs_loss':
        assert poison.compare(clean, dirty) == []                       # fixed-order reductions: the same bits
    else:
        for a, b in zip(clean, dirty):                                  # torch's own reductions may reorder: the same values to fp32 rounding
            torch.testing.assert_close(a, b, rtol=1e-5, atol=0)
    assert not poison.has_nan(dirty)


def test_workspace_buffer_reused_between_shapes():
    """The caching allocator hands the second call the first call's blocks: results equal a fresh process's (a clean call after empty_cache)."""
    from arlib_amd import allpairs as ap
    big, small = on_device(*problem(9001, 333, 64, 5, 0.15, seed=1)), on_device(*problem(700, 333, 64, 5, 0.15, seed=2))
    torch.cuda.empty_cache()
    alone = ap.bce_allpairs_loss(*small, want_grad=True)
    ap.bce_allpairs_loss(*big, want_grad=True)
    after = ap.bce_allpairs_loss(*small, want_grad=True)
    assert poison.compare(alone, after) == []


def test_one_attack_epoch_is_independent_of_scratch_memory():
    def epoch():
        data, args, params, noises = attack_problem(epochs=1)
        atk, _, res = run_device_attack(data, args, params, noises)
        return dict(loss=atk.loss_log, dS=atk.first_dS, picks=atk.pick_log, fake=res[300:].toarray(),
                    tables=[p.detach().clone() for p in atk.ngcf.parameters()])
    clean = epoch()
    with poison.poisoned_allocations():
        dirty = epoch()
    assert poison.compare(clean, dirty) == []
    assert not poison.has_nan(dirty)
