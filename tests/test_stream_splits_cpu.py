"""The host rules that cut a streamed table into splits (csrc/arl_stream.h and the families' own), without a GPU: the plain-Python restatement of
tests/stream_splits_restatement.py is pinned to the built library through the workspace sizes it exports, the restated rules keep their invariants
over the same sweep, and every shape a GPU test names for its split structure has that structure.  What the sizes cannot tell (no split length
enters one) is said in the restatement's docstring."""
import itertools

import stream_splits_restatement as S

LIMIT = S.ROW_LIMIT
# every threshold of every rule with a value on either side: the row floors 256 (unif), 512 (rank), 1 024 (stage_splits, ph_item_splits) and 4 096
# (split_count) and their doubles; the stage (64); the knee where the resident side alone fills the chip (2 048 workgroups of 64 rows = 131 072
# rows, 1 024 = 65 536 for the rank kernel) and the last resident size below it that still asks for two splits (64 * 2 047, 64 * 1 023); the
# streamed sizes at which a cap binds (64 * 512, 256 * 1 024, 256 * 4 096, 512 * 256) and the last one below (63 * 512, 255 * 1 024, 255 * 4 096);
# 1, the row limit and one past it
ROWS = sorted(set(v + o for v in (64, 256, 512, 1024, 2048, 4096, 8192, 64 * 1023, 65536, 64 * 2047, 131072, 63 * 512, 64 * 512, 255 * 1024, 256 * 1024,
                                   255 * 4096, 256 * 4096) for o in (-1, 0, 1)) | {1, 2, 3, 5793, LIMIT - 1, LIMIT, LIMIT + 1})
PAIRS = list(itertools.product(ROWS, ROWS))
VALID = [r for r in ROWS if r <= LIMIT]


def two_sided():
    """(rule name, n_streamed, (ns, len)) over the sweep, each rule with its own argument order."""
    for a, b in itertools.product(VALID, VALID):
        yield 'split_count', b, S.split_count(a, b)
        yield 'stage_splits', b, S.stage_splits(a, b)
        yield 'trk_splits', b, S.trk_splits(a, b)
    for n in VALID:
        yield 'ph_item_splits', n, S.ph_item_splits(n)
        if n >= 2:
            yield 'unif_splits', n, S.unif_splits(n)


def test_sweep_covers_the_thresholds():
    for v in (256, 257, 512, 513, 1024, 1025, 4096, 4097, 64, 131072, 131073, 1, LIMIT, LIMIT + 1):
        assert v in ROWS
    # the caps are reached inside the sweep, not only named
    assert max(S.split_count(a, b)[0] for a, b in PAIRS if max(a, b) <= LIMIT) == 256
    assert max(S.stage_splits(a, b)[0] for a, b in PAIRS if max(a, b) <= LIMIT) == 256
    assert max(S.trk_splits(a, b)[0] for a, b in PAIRS if max(a, b) <= LIMIT) == 64
    assert max(S.ph_item_splits(n)[0] for n in VALID) == 256
    # unif_splits' cap of 512 cannot bind: the table is both sides, and the two terms cross near n = 5 793 at 23 splits
    assert max(S.unif_splits(n)[0] for n in range(2, 20000)) == 23 == S.unif_splits(5793)[0]


def test_restated_sizes_equal_the_librarys():
    from arlib_amd import _lib
    L = _lib.lib()
    families = (('multinomial', L.arl_multinomial_softmax_workspace_bytes, S.multinomial_softmax_workspace_bytes),
                ('policy head', L.arl_bernoulli_softmax_workspace_bytes, S.bernoulli_softmax_workspace_bytes),
                ('column softmax', L.arl_colsoftmax_target_workspace_bytes, S.colsoftmax_target_workspace_bytes),
                ('all-pairs BCE', L.arl_bce_allpairs_workspace_bytes, S.bce_allpairs_workspace_bytes))
    bad, points = [], 0
    for (a, b), d, grad in itertools.product(PAIRS, S.WIDTHS, (0, 1)):
        for name, compiled, restated in families:
            points += 1
            got, want = int(compiled(a, b, d, grad)), restated(a, b, d, bool(grad))
            if got != want:
                bad.append((name, a, b, d, grad, got, want))
    for (a, b), d, T in itertools.product(PAIRS, S.WIDTHS, (1, 8, 9, 64)):
        points += 1
        got, want = int(L.arl_target_rank_workspace_bytes(a, b, d, T)), S.target_rank_workspace_bytes(a, b, d, T)
        if got != want:
            bad.append(('target rank', a, b, d, T, got, want))
    for n in ROWS + list(range(2, 20000, 37)):
        points += 1
        got, want = int(L.arl_uniformity_splits(n)), S.uniformity_splits(n)
        if got != want:
            bad.append(('uniformity', n, got, want))
    print('split rules pinned at %d points, %d mismatches' % (points, len(bad)))
    assert bad == [], bad[:5]
    # outside the shapes the sizes are 0 (the column softmax checks no upper limit: the restatement's docstring)
    for name, compiled, restated in families:
        assert compiled(0, 64, 16, 1) == restated(0, 64, 16, True) == 0 and compiled(64, 64, 24, 1) == restated(64, 64, 24, True) == 0, name
    assert L.arl_target_rank_workspace_bytes(3, 4097, 64, 0) == 0 == L.arl_target_rank_workspace_bytes(3, 4097, 64, 65)
    assert S.target_rank_workspace_bytes(3, 4097, 64, 0) == 0 == S.target_rank_workspace_bytes(3, 4097, 64, 65)


def test_a_size_moves_with_every_split_count():
    """The pinning can see each count: a size with one count changed differs from the true one wherever the count enters it."""
    B, I, d = S.BOTH_SPLIT_SHAPE
    mn, ph = S.mn_plan(B, I, d, True), S.ph_plan(B, I, d, True)
    u = S.up16
    assert mn['part_ms'] == u(4 * 2 * 3 * B) and mn['part_dq'] == u(4 * 3 * B * d) and mn['part_dE'] == u(4 * 2 * I * d)
    assert ph['part_ms'] == u(4 * 2 * 3 * B) and ph['part_sum'] == u(8 * 3 * 3 * B) and ph['part_dq'] == u(4 * 3 * B * d) and ph['part_dE'] == u(4 * 2 * I * d)
    one = S.ph_plan(3, 77, 16, True)
    assert one['part_dq'] == one['part_dE'] == 0                                     # one split writes the output itself
    assert S.csm_layout(4097, 65, 32, True)['gpart'] == S.up16(4 * 2 * 65 * 32) == S.bce_allpairs_workspace_bytes(4097, 65, 32, True)
    assert S.target_rank_workspace_bytes(3, 4097, 64, 8) == S.up16(4 * 9 * 3 * 8) and S.target_rank_workspace_bytes(200, 400, 64, 8) == 0


def test_every_row_lies_in_exactly_one_split_and_no_split_is_empty():
    seen = set()
    for rule, n, (ns, length) in two_sided():
        if (rule, n, ns, length) in seen:
            continue
        seen.add((rule, n, ns, length))
        assert 1 <= ns <= S.CAPS[rule], (rule, n, ns)
        assert (ns - 1) * length < n <= ns * length, (rule, n, ns, length)
        if rule in S.WHOLE_STAGE:
            assert length % 64 == 0, (rule, n, length)
        # the kernels' own bounds: split k takes [k len, min(n, (k + 1) len))
        sizes = [min(n, (k + 1) * length) - k * length for k in range(ns)]
        assert min(sizes) >= 1 and sum(sizes) == n and sizes[-1] == S.last_len(n, (ns, length)), (rule, n, ns, length)
    assert {r for r, _, _, _ in seen} == set(S.CAPS)


def test_row_floors_hold():
    """No rule cuts a split shorter than its floor allows: ns <= ceil(n / floor)."""
    floors = {'split_count': 4096, 'stage_splits': 1024, 'ph_item_splits': 1024, 'trk_splits': 512, 'unif_splits': 256}
    for rule, n, (ns, _) in two_sided():
        assert ns <= S.cdiv(n, floors[rule]), (rule, n, ns)
    for f, rule in ((4096, S.split_count), (1024, S.stage_splits), (512, S.trk_splits)):
        assert rule(1, f)[0] == 1 and rule(1, f + 1)[0] == 2                        # the smallest table that splits
    assert S.ph_item_splits(1024)[0] == 1 and S.ph_item_splits(1025)[0] == 2
    assert S.unif_splits(256)[0] == 1 and S.unif_splits(257)[0] == 2


def test_item_splits_of_the_policy_head_depend_on_the_items_alone():
    import inspect
    assert list(inspect.signature(S.ph_item_splits).parameters) == ['I']
    from arlib_amd import _lib
    L = _lib.lib()
    for I in VALID:
        si = S.ph_item_splits(I)[0]
        # part_ms [si][B][2] floats + stat + part_sum [si][B][3] doubles + tt without gradients: B = 4 keeps every section a multiple of 16 bytes, so
        # the library's own size gives si back whatever B's row blocks would make of stage_splits
        for B in (4, 4096, 131072):
            assert int(L.arl_bernoulli_softmax_workspace_bytes(B, I, 16, 0)) == (8 * si + 8 + 24 * si + 4) * B, (B, I)


def test_seam_rows():
    assert S.seam_rows(1025, (2, 576)) == [575, 576, 1024]
    assert S.seam_rows(1152, (2, 576)) == [575, 576, 1151]
    assert S.seam_rows(2049, (3, 704)) == [703, 704, 1407, 1408, 2048]
    assert S.seam_rows(77, (1, 128)) == [76]


def test_named_shapes_have_the_split_structure_claimed_for_them():
    for (B, I, d), (sb, last) in S.ROW_SPLIT_SHAPES.items():
        assert S.stage_splits(I, B) == sb and S.last_len(B, sb) == last, (B, I, d)
    # (1025, 70): the smallest B that splits, 7 stages and one live row in the last split; (1152, 33): the last split full; (2049, 65): 10 stages + 1
    assert S.stage_splits(70, 1024)[0] == 1 and 449 == 7 * 64 + 1 and 576 == 9 * 64 and 641 == 10 * 64 + 1
    B, I, d = S.BOTH_SPLIT_SHAPE
    sq, last = S.BOTH_ITEM_SPLIT
    assert S.stage_splits(B, I) == S.ph_item_splits(I) == sq and S.last_len(I, sq) == last
    for (B, I, d) in set(S.ROW_SPLIT_SHAPES) - {S.BOTH_SPLIT_SHAPE}:
        assert S.stage_splits(B, I)[0] == S.ph_item_splits(I)[0] == 1
    for (U, I), (split, last) in S.RANK_SPLIT_SHAPES.items():
        assert S.trk_splits(U, I) == split and S.last_len(I, split) == last, (U, I)
    for (U, I), ns in S.USER_SPLIT_COUNTS.items():
        assert S.split_count(I, U)[0] == ns, (U, I)
    assert S.split_count(65, 4097) == (2, 2049) and 2049 == 32 * 64 + 1 and 2049 % 4 != 0      # split 0 ends one row into its 33rd stage
    assert S.split_count(65, 4096)[0] == 1                                                    # the smallest table that splits
    for (B, I), split in S.ITEM_SPLITS.items():
        assert S.stage_splits(B, I) == S.ph_item_splits(I) == split, (B, I)

