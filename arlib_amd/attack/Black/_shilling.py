"""ShillingAttackModel (reference attack/Black/RandomAttack.py:7-66, repeated in BandwagonAttack.py): the data-only shilling attacks' base.

The reference draws every fake user's fillers with `random.sample(set(range(I)) - set(...), k)`.  Python 3.10 turns the set into a tuple, and
the iteration order of a set of small non-negative ints is ascending, so the draw is `random.sample(range(n), k)` mapped through the ascending
list of the remaining ids: `filler_draw` builds that list once and draws the indices with `sampler.sample_range` (same values, same MT19937
consumption).  That also works on Python >= 3.11, where `random.sample` of a set raises."""
import numpy as np
import scipy.sparse as sp

from .._common import AttackBase
from ...util.sampler import sample_range


class ShillingAttackModel(AttackBase):
    recommenderGradientRequired = False
    recommenderModelRequired = False

    def getPopularItemId(self, N):
        """N most popular items by feedback count: numpy's (unstable) argsort of the 1 x I sum, called as the reference calls it."""
        return np.argsort(self.interact[:, :].sum(0))[0, -N:].tolist()[0]

    def getReversePopularItemId(self, N):
        return np.argsort(self.interact[:, :].sum(0))[0, :N].tolist()[0]

    def posionDataAttack(self):
        """A rating matrix for the fake user segment (overridden by the attacks)."""


def remaining_ids(n, *excluded):
    """Ascending ids of range(n) minus every excluded id: the tuple CPython 3.10 makes of `set(range(n)) - set(a) - set(b)`."""
    keep = np.ones(int(n), bool)
    for ex in excluded:
        if len(ex):
            keep[np.asarray(ex, np.int64)] = False
    return np.flatnonzero(keep)


def filler_draw(pool, k):
    """random.sample(tuple(pool), k) for an ascending id array `pool`."""
    return pool[sample_range(len(pool), k)].tolist()


def fake_block(rows_cols, n_rows, n_items):
    """csr_matrix((ones, (row, col)), float32) of the reference's row/col lists: duplicate (row, col) pairs sum to 2.0."""
    row = np.concatenate([np.full(len(c), r, np.int64) for r, c in enumerate(rows_cols)]) if rows_cols else np.zeros(0, np.int64)
    col = np.concatenate([np.asarray(c, np.int64) for c in rows_cols]) if rows_cols else np.zeros(0, np.int64)
    return sp.csr_matrix((np.ones(len(col), np.int64), (row, col)), shape=(n_rows, n_items), dtype=np.float32)
