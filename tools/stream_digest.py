#!/usr/bin/env python3
"""SHA-256 digests of what the eight streamed-tile kernel families (arlib_amd/csrc/arl_stream.h) compute, to compare two builds of the library bit
for bit.  Every family is documented as deterministic (no atomics), so two libraries that order their arithmetic alike agree in every digest.

    python3 tools/stream_digest.py LIB            one line "<case> <tensor> <sha256>" per output tensor of the library at LIB
    python3 tools/stream_digest.py LIB_A LIB_B    one fresh child process per library (ARLIB_AMD_LIB selects it; the two are never loaded into one
                                                  process and this parent never touches the GPU), the digests diffed; exit status 1 on any difference

A library of another commit, for instance the parent of a refactor:
    git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/arlib_amd/csrc && python3 tools/stream_digest.py /tmp/parent/arlib_amd/lib/libarlib_amd.so arlib_amd/lib/libarlib_amd.so

Shapes are the smallest at which the shared tile code can go wrong: every width, 77 resident rows (a partial 16-row wave and a partial 64-row
workgroup), 5 streamed rows (one partial stage), and a streamed count that gives each family's own split rule at least two splits whose last one
ends in a partial stage: 2 100 where a split holds at least 1 024 (or 512) streamed rows, 8 300 where it holds 4 096, 257 rows for the square
uniformity kernel (at least 256 rows a split)."""
import hashlib
import os
import subprocess
import sys

WIDTHS = (16, 32, 64, 128)
N_RES = 77


def _digests():
    import torch
    from arlib_amd import ops, colsoftmax, cluster, pairloss, allpairs, policyhead, targetrank, multinomial
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(20240607)
    out = []

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=gen) * scale).to(dev)

    def unit(n, d):
        return torch.nn.functional.normalize(torch.randn(n, d, generator=gen), dim=1).to(dev).contiguous()

    def csr(rows, cols, per_row, weights):
        """per_row distinct sorted columns for every row; (rowptr, col[, val]) int32 / fp32 on the device"""
        k = min(per_row, cols)
        col = torch.stack([torch.randperm(cols, generator=gen)[:k].sort().values for _ in range(rows)]).reshape(-1).to(torch.int32)
        rowptr = (torch.arange(rows + 1) * k).to(torch.int32)
        pos = (rowptr.to(dev), col.to(dev))
        return pos + ((torch.rand(rows * k, generator=gen) + 0.5).to(dev),) if weights else pos

    def emit(case, names, tensors):
        torch.cuda.synchronize()
        for name, t in zip(names, tensors):
            if t is not None:
                out.append('%s %s %s' % (case, name, hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()))

    for d in WIDTHS:
        for n_str in (5, 8300):                        # 4 096 streamed rows a split: nce_allrows, colsoftmax, bce_allpairs
            A, V = unit(N_RES, d), unit(n_str, d)
            emit('nce_allrows/d%d/t%d/lse' % (d, n_str), ('lse',), (ops.nce_allrows(A, V, 0.2, want_grad=False),))
            emit('nce_allrows/d%d/t%d/grad' % (d, n_str), ('lse', 'dA', 'dV'), ops.nce_allrows(A, V, 0.2))
            emit('nce_allrows/d%d/t%d/grad_no_dV' % (d, n_str), ('lse', 'dA'), ops.nce_allrows(A, V, 0.2, want_dV=False)[:2])
            Pu, Pi = rnd(n_str, d, scale=0.3), rnd(N_RES, d, scale=0.3)          # the users are the streamed side of the split passes
            emit('colsoftmax/d%d/t%d' % (d, n_str), ('loss', 'lse', 'dPu', 'dPi'), colsoftmax.colsoftmax_target_loss(Pu, Pi, [3, 70, 3], want_grad=True))
            pos, rw = csr(n_str, N_RES, 3, True), (torch.rand(n_str, generator=gen) + 0.5).to(dev) / n_str
            emit('bce_allpairs/d%d/t%d/loss' % (d, n_str), ('loss', 'rowloss'), allpairs.bce_allpairs_loss(Pu, Pi, pos, rw))
            emit('bce_allpairs/d%d/t%d/grad' % (d, n_str), ('loss', 'rowloss', 'dPu', 'dPi'), allpairs.bce_allpairs_loss(Pu, Pi, pos, rw, want_grad=True, upstream=0.7))
        for n_str in (5, 2100):                        # 1 024 (target rank: 512) streamed rows a split, whole stages; k-means streams the centroids whole
            X, C = rnd(N_RES, d), rnd(n_str, d)
            emit('kmeans_assign/d%d/t%d' % (d, n_str), ('labels', 'score'), cluster.kmeans_assign(X, C))
            q, E = rnd(N_RES, d, scale=0.3), rnd(n_str, d, scale=0.3)
            act = policyhead.pack_bits((torch.rand(N_RES, n_str, generator=gen) < 0.3).to(dev))
            gl, ge = rnd(N_RES), rnd(N_RES)
            emit('bernoulli_eval/d%d/t%d' % (d, n_str), ('logp', 'ent', 'dq', 'dE'), policyhead.bernoulli_softmax_eval(q, E, act, gl, ge, want_grad=True))
            emit('bernoulli_sample/d%d/t%d' % (d, n_str), ('actions', 'logp', 'count'), policyhead.bernoulli_softmax_sample(q, E, seed=11, call=3, row0=5))
            targets = torch.tensor([0, n_str - 1, n_str // 2], dtype=torch.int32, device=dev)
            emit('target_rank/d%d/t%d' % (d, n_str), ('rank', 'tscore'), targetrank.target_rank_kernel(q, E, targets, csr(N_RES, n_str, 4, False)))
            emit('multinomial/d%d/t%d' % (d, n_str), ('nll', 'lse', 'dq', 'dE'),
                 multinomial.multinomial_softmax_kernel(q, E, csr(N_RES, n_str, 4, True), g=rnd(N_RES), want_grad=True))
        for n in (5, N_RES, 257):                      # the square kernel: 257 is the smallest n with two splits
            x = rnd(n, d)
            emit('uniformity/d%d/n%d/fwd' % (d, n), ('loss',), pairloss.uniformity(x, 2, want_grad=False)[:1])
            emit('uniformity/d%d/n%d/bwd' % (d, n), ('loss', 'dX'), pairloss.uniformity(x, 2, want_grad=True, upstream=0.5))
    return out


def _child(lib):
    env = dict(os.environ, ARLIB_AMD_LIB=os.path.abspath(lib))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--run'], env=env, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit('stream_digest: the run of %s ended with status %d' % (lib, r.returncode))
    return [ln for ln in r.stdout.splitlines() if ln.count(' ') == 2]


def main(argv):
    if argv == ['--run']:                              # the child: the library is the one ARLIB_AMD_LIB names
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
        print('\n'.join(_digests()))
        return 0
    if len(argv) not in (1, 2) or not all(os.path.isfile(p) for p in argv):
        sys.exit(__doc__)
    runs = [_child(p) for p in argv]
    if len(runs) == 1:
        print('\n'.join(runs[0]))
        return 0
    a, b = runs
    keys = lambda ls: [ln.rsplit(' ', 1)[0] for ln in ls]
    if keys(a) != keys(b):
        sys.exit('stream_digest: the two runs list different tensors')
    diff = [(x, y) for x, y in zip(a, b) if x != y]
    for x, y in diff:
        print('DIFF %s\n     %s' % (x, y.rsplit(' ', 1)[1]))
    print('stream_digest: %d tensors, %d differ' % (len(a), len(diff)))
    return 1 if diff else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
