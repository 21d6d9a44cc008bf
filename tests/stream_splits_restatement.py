"""Plain-Python restatement of the host rules that cut a streamed table into splits, and of the workspace layouts those split counts enter.  A
helper, not collected; no import of the product.

Every rule returns (ns, len): the number of splits and the streamed rows of each but the last; split k takes the rows [k len, min(n, (k + 1) len)).

    split_count(n_resident, n_streamed)   csrc/arl_stream.h, used by arl_allpairs.hip (items resident, users streamed) and arl_colsoftmax.hip
    stage_splits(n_resident, n_streamed)  csrc/arl_stream.h: the multinomial's and the policy head's sq = (B, I) and sb = (I, B)
    ph_item_splits(I)                     csrc/arl_policyhead.hip: the statistics, row-sum and sampling passes
    trk_splits(U, I)                      csrc/arl_targetrank.hip
    unif_splits(n)                        csrc/arl_pairloss.hip (the table is both sides)

stage_splits, ph_item_splits and trk_splits cut whole 64-row stages (WHOLE_STAGE); split_count and unif_splits cut ceil(n / ns) rows.

What the library's exported sizes can and cannot tell (tests/test_stream_splits_cpu.py compares them point by point):
  * every split COUNT enters a size: sq.ns and sb.ns of the multinomial (part_ms, part_dq, part_dE), si.ns, sq.ns and sb.ns of the policy head
    (the last two only where they exceed 1: one split writes the output itself), split_count through arl_bce_allpairs_workspace_bytes and
    arl_colsoftmax_target_workspace_bytes, trk_splits' count (0 bytes at one split) and unif_splits through arl_uniformity_splits itself;
  * NO split LENGTH enters any size.  The lengths here are restated from the sources and are tied to the compiled rules only through the counts
    (ns = ceil(n / len) for the whole-stage rules): a length that is wrong here and gives the same count would pass the pinning.  What the GPU tests
    assert about a last split's length therefore rests on this file's reading of the rule, not on the library's answer;
  * arl_colsoftmax_target_workspace_bytes checks no upper row limit (the op itself refuses such a call), the other four return 0 past it: restated
    as they are."""

ROW_LIMIT = (2 ** 31 - 1) // 128
WIDTHS = (16, 32, 64, 128)
WHOLE_STAGE = ('stage_splits', 'ph_item_splits', 'trk_splits')
CAPS = {'split_count': 256, 'stage_splits': 256, 'ph_item_splits': 256, 'trk_splits': 64, 'unif_splits': 512}


def cdiv(a, b):
    return -(-a // b)


def up16(b):
    return (b + 15) // 16 * 16


def _whole_stages(n, s):
    length = cdiv(cdiv(n, s), 64) * 64
    return cdiv(n, length), length


def split_count(n_resident, n_streamed):
    """At least 4 096 streamed rows a split, 2 048 workgroups aimed at, 256 splits at most; the callers stream ceil(n / ns) rows a split."""
    s = min(cdiv(2048, cdiv(n_resident, 64)), cdiv(n_streamed, 4096), 256)
    s = max(s, 1)
    return s, cdiv(n_streamed, s)


def stage_splits(n_resident, n_streamed):
    """At least 1 024 streamed rows a split, 2 048 workgroups aimed at, 256 splits at most, whole stages."""
    s = min(cdiv(2048, cdiv(n_resident, 64)), cdiv(n_streamed, 1024), 256)
    return _whole_stages(n_streamed, max(s, 1))


def ph_item_splits(I):
    """At least 1 024 items a split, 256 splits at most, whole stages: a function of I alone."""
    return _whole_stages(I, min(cdiv(I, 1024), 256))


def trk_splits(U, I):
    """At least 512 items a split, 1 024 workgroups aimed at, 64 splits at most, whole stages."""
    s = min(cdiv(1024, cdiv(U, 64)), cdiv(I, 512), 64)
    return _whole_stages(I, max(s, 1))


def unif_splits(n):
    """At least 256 rows a split, 2 048 workgroups aimed at, 512 splits at most; ceil(n / ns) rows a split."""
    s = min(cdiv(2048, cdiv(n, 64)), cdiv(n, 256), 512)
    s = max(s, 1)
    return s, cdiv(n, s)


def uniformity_splits(n):
    """arl_uniformity_splits: the count, 0 outside 2 <= n <= ROW_LIMIT."""
    return unif_splits(n)[0] if 2 <= n <= ROW_LIMIT else 0


def last_len(n, split):
    """Rows of the last split."""
    ns, length = split
    return n - (ns - 1) * length


def seam_rows(n, split):
    """The last row of every split, the first row of the next, and row n - 1, ascending."""
    ns, length = split
    rows = set([n - 1])
    for k in range(1, ns):
        rows |= {k * length - 1, k * length}
    return sorted(rows)


# ---------------------------------------------------------------------------------------- the shapes the GPU tests name for their split structure
# test_gpu_stream_splits.py, (B, I, d) -> sb = stage_splits(I, B) and the rows of its last split: the batch rows streamed in splits
ROW_SPLIT_SHAPES = {(1025, 70, 16): ((2, 576), 449), (1152, 33, 128): ((2, 576), 576), (2049, 65, 64): ((3, 704), 641), (1089, 2049, 32): ((2, 576), 513)}
# the one of them that also splits the items: sq = stage_splits(B, I) = si = ph_item_splits(I) and the items of the last split
BOTH_SPLIT_SHAPE, BOTH_ITEM_SPLIT = (1089, 2049, 32), ((3, 704), 641)
# test_gpu_stream_splits.py, (U, I) -> trk_splits(U, I) and the items of the last split
RANK_SPLIT_SHAPES = {(3, 4097): ((9, 512), 1), (17, 1025): ((3, 384), 257)}
# test_gpu_gsp.py and test_gpu_legup.py, (streamed users, resident items) -> split_count; every other shape of theirs is one split
USER_SPLIT_COUNTS = {(9001, 130): 3, (20000, 70): 5, (4097, 65): 2}
# test_gpu_multinomial.py and test_gpu_policyhead.py, (B, I) -> stage_splits(B, I) = ph_item_splits(I); every other shape of theirs is one split
ITEM_SPLITS = {(130, 1030): (2, 576), (33, 4099): (5, 832)}


def shape_ok(n_a, n_b, d):
    return d in WIDTHS and 0 < n_a <= ROW_LIMIT and 0 < n_b <= ROW_LIMIT


# ---------------------------------------------------------------------------------------- workspace layouts: section name -> bytes, in order
def mn_plan(B, I, d, grad):
    sq, sb = stage_splits(B, I), stage_splits(I, B)
    L = {'part_ms': up16(4 * 2 * sq[0] * B), 'stat': up16(4 * 2 * B), 'coef': up16(4 * B)}
    L['part_dq'] = up16(4 * sq[0] * B * d) if grad else 0
    L['part_dE'] = up16(4 * sb[0] * I * d) if grad else 0
    return L


def ph_plan(B, I, d, grad):
    si, sq, sb = ph_item_splits(I), stage_splits(B, I), stage_splits(I, B)
    L = {'part_ms': up16(4 * 2 * si[0] * B), 'stat': up16(4 * 2 * B), 'part_sum': up16(8 * 3 * si[0] * B), 'tt': up16(4 * B)}
    L['part_dq'] = up16(4 * sq[0] * B * d) if grad and sq[0] > 1 else 0
    L['part_dE'] = up16(4 * sb[0] * I * d) if grad and sb[0] > 1 else 0
    return L


def csm_layout(U, I, d, want_dPi):
    ns = split_count(I, U)[0]
    chunks = min(max(cdiv(U, 1024), 1), 1024)
    L = {'colpart': up16(8 * chunks * d), 'head': up16(8 * 2), 'lpart': up16(8 * cdiv(I, 256)), 'sub_u': up16(4 * d), 'sub_i': up16(4 * d),
         'pm': up16(4 * ns * I), 'ps': up16(4 * ns * I)}
    L['gpart'] = up16(4 * ns * I * d) if want_dPi else 0
    return L


def multinomial_softmax_workspace_bytes(B, I, d, grad):
    return sum(mn_plan(B, I, d, grad).values()) if shape_ok(B, I, d) else 0


def bernoulli_softmax_workspace_bytes(B, I, d, grad):
    return sum(ph_plan(B, I, d, grad).values()) if shape_ok(B, I, d) else 0


def colsoftmax_target_workspace_bytes(U, I, d, want_dPi):
    return sum(csm_layout(U, I, d, want_dPi).values()) if U > 0 and I > 0 and d in WIDTHS else 0


def bce_allpairs_workspace_bytes(R, I, d, grad):
    if not shape_ok(R, I, d) or not grad:
        return 0
    return up16(4 * split_count(I, R)[0] * I * d)


def target_rank_workspace_bytes(U, I, d, T):
    if not shape_ok(U, I, d) or not 1 <= T <= 64:
        return 0
    ns = trk_splits(U, I)[0]
    return up16(4 * ns * U * T) if ns > 1 else 0
