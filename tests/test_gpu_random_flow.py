"""The reference's default ARLib.py flow (conf/attack_parser.py: attackModelName = RandomAttack) on the drop-in classes: LightGCN trained and
tested, RandomAttack's poison data written with dataSave and read back through the file DataLoader, the victim re-initialised on it, retrained
and tested, AttackMetric on the targets (ARLib.py:92-236)."""
import contextlib
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
from conftest import golden
from test_host_api import make_data

pytestmark = pytest.mark.gpu


def rec_args(**kw):
    a = dict(dataset='ml-100k', data_path='', training_data='', val_data='', test_data='', model_name='LightGCN', maxEpoch=1, batch_size=2048,
             emb_size=32, n_layers=2, reg=1e-4, lRate=0.005, seed=2018, topK='10,50')
    a.update(kw)
    return SimpleNamespace(**a)


def test_default_flow_lightgcn_with_random_attack(tmp_path, monkeypatch):
    from arlib_amd.util.tool import seedSet, dataSave
    from arlib_amd.util.DataLoader import DataLoader
    from arlib_amd.util.FileIO import FileIO
    from arlib_amd.util.metrics import AttackMetric
    from arlib_amd.recommender.LightGCN import LightGCN
    from arlib_amd.attack.Black.RandomAttack import RandomAttack
    monkeypatch.chdir(tmp_path)
    seedSet(2018)
    data = make_data()
    rec = LightGCN(rec_args(), data)
    atk_args = SimpleNamespace(maliciousUserSize=0.01, maliciousFeedbackSize=0, Epoch=1, innerEpoch=1, outerEpoch=1,
                               attackTargetChooseWay='unpopular', targetSize=5)
    atk = RandomAttack(atk_args, data)
    assert atk.recommenderModelRequired is False and atk.recommenderGradientRequired is False
    with contextlib.redirect_stdout(io.StringIO()):
        rec.train()
        _, raw = rec.test()
    poison = sp.csr_matrix(atk.posionDataAttack())                       # no recommender argument (ARLib.py:230-231)
    U, F = data.user_num, atk.fakeUserNum
    assert poison.shape == (U + F, data.item_num) and (poison[:U] != sp.csr_matrix(data.matrix())).nnz == 0
    assert (poison[U:].getnnz(1) == atk.maliciousFeedbackNum + len(atk.targetItem)).all()
    out_dir = 'data/poison/RandomAttack_ml-100k/0/'
    os.makedirs(out_dir, exist_ok=True)
    dataSave(poison, out_dir + 'train.txt', data.id2user, data.id2item)
    g = golden('ml100k_data.npz')
    for name in ('val', 'test'):
        FileIO.write_file(out_dir, name + '.txt', ['%d %d %s\n' % (a, b, c) for a, b, c in zip(g[name + '_u'].tolist(), g[name + '_i'].tolist(), g[name + '_r'].tolist())])
    pargs = rec_args(dataset='RandomAttack_ml-100k/0', data_path='data/poison/', training_data='/train.txt', val_data='/val.txt', test_data='/test.txt')
    pdata = DataLoader(pargs)
    assert pdata.user_num == U + F and pdata.item_num == data.item_num and sp.csr_matrix(pdata.matrix()).nnz == poison.nnz
    rec.__init__(pargs, pdata)                                           # ARLib.py:137: same object, poisoned data
    with contextlib.redirect_stdout(io.StringIO()):
        rec.train()
        _, after = rec.test()
    assert len(after) == len(raw) and after[0] == raw[0] == 'Top 10\n'
    hr = AttackMetric(rec, atk.targetItem, [10, 50]).hitRate()
    assert len(hr) == 2 and all(0.0 <= x <= 1.0 for x in hr) and hr[0] <= hr[1] + 1e-12
