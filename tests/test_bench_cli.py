"""bench.py's command line without a GPU: argument checks and the row sample --dump-outputs writes."""
import os
import subprocess
import sys
import numpy as np
import pytest
from conftest import ROOT

import bench


@pytest.mark.parametrize('U,I,d', [(1_000_000, 100_000, 64), (1_000_000, 100_000, 128), (10_000_000, 1_000_000, 128), (30_000, 3_000, 64), (200, 5_000_000, 64)])
def test_dump_rows_fit_the_budget_and_depend_on_the_arguments_only(U, I, d):
    ru, ri = bench.dump_rows(U, I, d, 2018)
    assert (len(ru) + len(ri)) * 4 * d + 4 * 4 + 3 * 128 <= bench.DUMP_BYTES           # the tables, the loss vector and the .npy headers
    for rows, n in ((ru, U), (ri, I)):
        assert rows.dtype == np.int64 and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n
    if U + I <= bench.DUMP_BYTES // (4 * d) - 16:
        assert len(ru) == U and len(ri) == I                                              # small tables go out whole
    else:
        assert len(ru) + len(ri) > 0.99 * (bench.DUMP_BYTES // (4 * d)) - 16                # a large table fills the budget
    ru2, ri2 = bench.dump_rows(U, I, d, 2018)
    assert np.array_equal(ru, ru2) and np.array_equal(ri, ri2)
    if len(ru) < U:
        assert not np.array_equal(bench.dump_rows(U, I, d, 7)[0], ru)


def test_cfg2_dump_keeps_every_item_row():
    ru, ri = bench.dump_rows(1_000_000, 100_000, 64, 2018)
    assert len(ri) == 100_000 and len(ru) > 100_000


@pytest.mark.parametrize('argv', [['--steps', '0'], ['--warmup', '-1']])
def test_bench_rejects_step_counts_without_a_timed_step(argv):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1'] + argv, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 2 and '--steps must be >= 1' in p.stderr
