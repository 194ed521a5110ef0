"""GPU: hgd_bpr_forward / hgd_bpr_backward called through the C ABI at the edges of csrc/bpr.hip.

The reference is tests/_bpr_ref64.py (float64 numpy, checked on the CPU by tests/test_bpr_ref.py).
Every array of every call — the table, the three id arrays, coef, grad, loss, anc_out, pos_out,
dE, the bad-index word and the workspace, given exactly hgd_bpr_workspace_size bytes — is carved
out of one guarded device buffer (tests/_arena.py); after every launch the guards and the inputs
must be bytewise unchanged. dE starts as the sentinel, so a row the backward forgets to write or
to zero shows, and the table lies directly between guards whose float value is -4.3e8, so a read
past it shows in the result.

The backward and the gathered rows are compared with ``==`` on exact_case data (every float32
product and partial sum exact in any order), never with a tolerance. What these batches reach in
bpr.hip, which functional.bpr_loss_rows on random contiguous tables never does:
  * every column-block form of group_for(d): lane groups of 1, 4, 16, 64 with 1 .. 4 float4
    blocks per lane and a ragged last block;
  * lde != d, ldd != d, lde != ldd, the zero-fill of a padded dE, NULL anc_out / pos_out /
    bad_index;
  * batches one short of, on and one past a block of lane groups, in B and in 3B;
  * heavy rows (more than kWalkMax = 8 positions) whose hits straddle a thread's 16 positions, a
    wave's 1,024 and a window's 4,096, a user row in two windows, a window without hits, fewer
    hits than lane groups, rows heavy only by positives plus negatives, more heavy rows than
    kHeavyGrid = 256 blocks and the heavy list filled to its capacity term 3B/9;
  * negative, out-of-range and extreme int64 ids.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from hypergraph_diffusion_for_recommendation_amd import _native as nat
from tests import _bpr_ref64 as R
from tests._arena import SENTINEL, Arena, bits

pytestmark = pytest.mark.gpu

WORKSPACE = 4  # HGD_ERR_WORKSPACE
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
TAIL = 4096  # sentinel bytes kept behind the workspace, the last array a call may write


def _sentinel(n, dtype):
    return np.full(n * np.dtype(dtype).itemsize, SENTINEL, dtype=np.uint8).view(dtype)


def _is_sentinel(x):
    return bool((np.ascontiguousarray(x).view(np.uint8) == SENTINEL).all())


def _strided(E, ld):
    """[N, d] as the flat (N - 1)·ld + d floats of a row-padded table; the padding is sentinel."""
    N, d = E.shape
    flat = _sentinel((N - 1) * ld + d, np.float32).copy()
    flat[(np.arange(N)[:, None] * ld + np.arange(d)).ravel()] = E.ravel()
    return flat


def _unstrided(flat, N, d, ld):
    """(the [N, d] values, the padding between the rows) of a flat row-padded table."""
    at = np.arange(N)[:, None] * ld + np.arange(d)
    pad = np.ones(flat.size, bool)
    pad[at.ravel()] = False
    return flat[at], flat[pad]


def _need(c):
    return nat.load().hgd_bpr_workspace_size(c.B, c.nu + c.ni)


def _ids(ar, c):
    for name in ("uid", "pid", "nid"):
        ar.add(name, getattr(c, name))
    return ar


def _forward(dev, c, lde=None, anc=True, pos=True, bad=True, bad0=0, calls=1, short=0,
             what="forward"):
    """Runs hgd_bpr_forward ``calls`` times; returns the outputs (and the status when the
    workspace is given ``short`` bytes fewer than it needs)."""
    lde = lde or c.d
    need = _need(c)
    ar = _ids(Arena().add("E", _strided(c.E, lde)), c)
    ar.add("coef", _sentinel(c.B, np.float32), out=True)
    ar.add("loss", _sentinel(1, np.float32), out=True)
    ar.add("anc", _sentinel(c.B * c.d, np.float32), out=True)
    ar.add("pos", _sentinel(c.B * c.d, np.float32), out=True)
    ar.add("bad", np.array([bad0], np.int32), out=True)
    ar.add("ws", _sentinel(need, np.uint8), out=True)
    ar.add("tail", _sentinel(TAIL, np.uint8))
    ar.upload(dev)
    lib = nat.load()
    for _ in range(calls):
        st = lib.hgd_bpr_forward(
            ar.ptr("E"), lde, c.nu, c.ni, c.d, ar.ptr("uid"), ar.ptr("pid"), ar.ptr("nid"), c.B,
            ar.ptr("anc") if anc else None, ar.ptr("pos") if pos else None, ar.ptr("coef"),
            ar.ptr("loss"), ar.ptr("bad") if bad else None, ar.ptr("ws"), need - short,
            nat.stream_handle(dev))
        if short:
            message = lib.hgd_get_last_error_string().decode()
            outs = ar.check(what)
            return st, message, outs
        nat.check(st, "hgd_bpr_forward")
    outs = ar.check(what)
    if not anc:
        assert _is_sentinel(outs["anc"]), what
    if not pos:
        assert _is_sentinel(outs["pos"]), what
    if not bad:
        assert outs["bad"].tolist() == [bad0], what
    return SimpleNamespace(anc=outs["anc"].reshape(c.B, c.d), pos=outs["pos"].reshape(c.B, c.d),
                           coef=outs["coef"], loss=outs["loss"][0], bad=int(outs["bad"][0]))


def _backward(dev, c, lde=None, ldd=None, runs=2, short=0, what="backward"):
    """Runs hgd_bpr_backward on c's coef and grad ``runs`` times, dE refilled with the sentinel
    before each: the runs must agree bitwise (the list order is timing-dependent by design, the
    sums are not) and leave dE's padding alone. Returns dE [N, d]."""
    lde, ldd = lde or c.d, ldd or c.d
    N = c.nu + c.ni
    need = _need(c)
    blank = _sentinel((N - 1) * ldd + c.d, np.float32)
    ar = _ids(Arena().add("E", _strided(c.E, lde)), c)
    ar.add("coef", c.coef).add("grad", c.grad)
    ar.add("dE", blank, out=True)
    ar.add("ws", _sentinel(need, np.uint8), out=True)
    ar.add("tail", _sentinel(TAIL, np.uint8))
    ar.upload(dev)
    lib = nat.load()
    got = []
    for run in range(runs):
        if run:
            ar.write("dE", blank)
        st = lib.hgd_bpr_backward(
            ar.ptr("E"), lde, c.nu, c.ni, c.d, ar.ptr("uid"), ar.ptr("pid"), ar.ptr("nid"), c.B,
            ar.ptr("coef"), ar.ptr("grad"), ar.ptr("dE"), ldd, ar.ptr("ws"), need - short,
            nat.stream_handle(dev))
        if short:
            message = lib.hgd_get_last_error_string().decode()
            outs = ar.check(what)
            return st, message, outs
        nat.check(st, "hgd_bpr_backward")
        dE, pad = _unstrided(ar.check((what, run))["dE"], N, c.d, ldd)
        assert _is_sentinel(pad), f"{what}: dE's padding was written"
        got.append(dE)
    for other in got[1:]:
        assert np.array_equal(bits(got[0]), bits(other)), f"{what}: two runs differ"
    return got[0]


def _assert_exact(dE, c, what):
    """dE == the float64 reference (exact in float32); values, so that -0 == +0."""
    wrong = np.argwhere(~(dE == c.dE))
    if wrong.size:
        r, col = (int(x) for x in wrong[0])
        rows = np.unique(wrong[:, 0])
        raise AssertionError(
            f"{what}: dE[{r}, {col}] = {dE[r, col]!r}, expected {c.dE[r, col]!r}; "
            f"{len(wrong)} entries in {rows.size} rows differ (rows {rows[:8].tolist()}, "
            f"hit counts {_counts(c)[rows[:8]].tolist()})")
    assert not dE[~c.touched].any(), f"{what}: a row no position names is not zero"


def _counts(c):
    """Positions naming each table row."""
    ru, _ = R.resolve(c.uid, c.nu)
    rp, _ = R.resolve(c.pid, c.ni)
    rn, _ = R.resolve(c.nid, c.ni)
    return np.bincount(np.concatenate([ru, c.nu + rp, c.nu + rn]), minlength=c.nu + c.ni)


def _check_forward_of_exact(dev, c, what, **kw):
    """The gathered rows bitwise; coef and loss within the bounds of the float tests below (the
    scores are exact multiples of 1/16, expf and logf are not)."""
    got = _forward(dev, c, what=what, **kw)
    assert np.array_equal(bits(got.anc), bits(c.anc)), f"{what}: anc_out"
    assert np.array_equal(bits(got.pos), bits(c.pos)), f"{what}: pos_out"
    ref = R.forward(c.E, c.nu, c.ni, c.uid, c.pid, c.nid)
    assert np.isfinite(got.coef).all() and np.isfinite(got.loss)
    assert np.abs(got.coef - ref.coef).max() <= 1e-5, what
    assert abs(got.loss - ref.loss) <= 1e-5 * np.mean(np.abs(ref.term) + 1), what
    assert got.bad == ref.bad_rows
    return got


def _background(rng, B, nu, ni, keep):
    """Valid ids that leave the first ``keep`` users and items to the test."""
    return [rng.integers(keep, n, B) for n in (nu, ni, ni)]


def _plant(rng, ids, plan):
    """ids[at] = row for ``count`` random free positions of each (row, count) of ``plan``."""
    free = rng.permutation(ids.size)
    used = 0
    for row, count in plan:
        ids[free[used:used + count]] = row
        used += count
    assert used <= ids.size


# ---- widths and padding -----------------------------------------------------------------------
WIDTHS = [4, 8, 12, 16, 48, 60, 64, 192, 252, 256]
REPEATS = (1, 2, 7, 8, 9, 10, 65)  # walked: at most kWalkMax = 8 positions; heavy: more


@functools.lru_cache(maxsize=None)
def _width_case(d):
    rng = np.random.default_rng(1000 + d)
    nu, ni, B, keep = 301, 397, 333, 20
    uid, pid, nid = _background(rng, B, nu, ni, keep)
    _plant(rng, uid, list(enumerate(REPEATS)))
    _plant(rng, pid, list(enumerate(REPEATS)))
    _plant(rng, nid, [(10 + j, n) for j, n in enumerate(REPEATS)])
    c = R.exact_case(rng, nu, ni, d, uid, pid, nid, m=d % 3)
    cnt = _counts(c)
    for j, n in enumerate(REPEATS):
        assert cnt[j] == cnt[nu + j] == cnt[nu + 10 + j] == n
    assert not c.touched.all() and np.abs(c.dE).max() > 1
    return c


@pytest.mark.parametrize("d", WIDTHS)
def test_every_width_forward(dev, d):
    _check_forward_of_exact(dev, _width_case(d), f"d = {d}")


@pytest.mark.parametrize("d", WIDTHS)
def test_every_width_backward(dev, d):
    """Users, positive items and negative items named 1, 2, 7 and 8 times (walked lists) and 9,
    10 and 65 times (the heavy kernel), among rows named a few times and rows never named."""
    c = _width_case(d)
    _assert_exact(_backward(dev, c, what=f"d = {d}"), c, f"d = {d}")


@pytest.mark.parametrize("d", WIDTHS)
def test_padded_rows(dev, d):
    """lde = d + 4, ldd = d + 8: dE[:, :d] exact, its padding still the sentinel (checked in
    _backward), unnamed rows exactly zero; the forward reads the padded table the same way."""
    c = _width_case(d)
    _check_forward_of_exact(dev, c, f"d = {d}, lde = d + 4", lde=d + 4)
    _assert_exact(_backward(dev, c, lde=d + 4, ldd=d + 8, what=f"padded d = {d}"), c,
                  f"padded d = {d}")
    _assert_exact(_backward(dev, c, ldd=d + 4, what=f"padded dE only, d = {d}"), c,
                  f"padded dE only, d = {d}")


# ---- batch edges per lane-group width ---------------------------------------------------------
def _edge_batches(gpb):
    """1, GPB - 1, GPB, GPB + 1 and the smallest B whose 3B positions end one or two short of a
    block of GPB lane groups, on one, and one or two past one."""
    below = next(B for B in range(1, gpb + 2) if 3 * B % gpb >= gpb - 2)
    on = next(B for B in range(1, gpb + 2) if 3 * B % gpb == 0)
    above = next(B for B in range(1, gpb + 2) if 3 * B > gpb and 3 * B % gpb in (1, 2))
    return sorted({1, gpb - 1, gpb, gpb + 1, below, on, above})


@pytest.mark.parametrize("d,G", [(8, 1), (16, 4), (64, 16), (256, 64)])
def test_batch_edges(dev, d, G):
    gpb = 256 // G
    batches = _edge_batches(gpb)
    assert {1, gpb - 1, gpb, gpb + 1} <= set(batches)
    rng = np.random.default_rng(d)
    nu, ni = 5, 3
    for B in batches:
        uid, pid, nid = _background(rng, B, nu, ni, 0)
        c = R.exact_case(rng, nu, ni, d, uid, pid, nid, m=1)
        _check_forward_of_exact(dev, c, f"d = {d}, B = {B}")
        _assert_exact(_backward(dev, c, what=f"d = {d}, B = {B}"), c, f"d = {d}, B = {B}")


# ---- heavy rows: windows, waves, threads ------------------------------------------------------
HEAVY_WIDTHS = [12, 60, 128, 256]  # one per lane-group width


@functools.lru_cache(maxsize=None)
def _user_window_case(d, B, second):
    rng = np.random.default_rng(B + d)
    nu, ni, keep = 700, 900, 4
    uid, pid, nid = _background(rng, B, nu, ni, keep)
    uid[4091:4100] = 0                      # 5 anchors in the first window, 4 in the second
    uid[[3, 17, 1023, 1024, 1500, 2047, 2048, 3000, 4090]] = 2   # first window only
    if second:
        uid[4100:4110] = 1                  # 10 anchors, all in the second window
    c = R.exact_case(rng, nu, ni, d, uid, pid, nid, m=2)
    cnt = _counts(c)
    assert cnt[0] == 9 and cnt[2] == 9 and cnt[1] == (10 if second else 0)
    return c


@pytest.mark.parametrize("d", HEAVY_WIDTHS)
def test_user_rows_across_windows(dev, d):
    """B = 4,100: a user row with 9 anchors at positions 4,091 .. 4,099, 5 hits in the first
    4,096-position window and 4 in the second, and a user row whose 9 hits leave the second
    window empty. Those 9 anchors fill the second window's 4 positions, so the user row whose
    hits ALL lie in the second window (its first window is the empty one) needs a longer batch:
    B = 4,110 with 10 more anchors at 4,100 .. 4,109."""
    for B, second in ((4100, False), (4110, True)):
        c = _user_window_case(d, B, second)
        _assert_exact(_backward(dev, c, what=f"user windows d = {d}, B = {B}"), c,
                      f"user windows d = {d}, B = {B}")


@functools.lru_cache(maxsize=None)
def _item_window_case(d):
    rng = np.random.default_rng(2100 + d)
    nu, ni, B, keep = 500, 800, 2100, 4
    uid, pid, nid = _background(rng, B, nu, ni, keep)
    # positions of the scanned range [B, 3B), relative to B: a thread's 16th and 17th, a wave's
    # 1,024th and 1,025th, the last positive and first negative, a window's last and the next
    # window's first, the last of all
    rel = [0, 15, 16, 1023, 1024, 2099, 2100, 4095, 4096, 2 * B - 1]
    for q in rel:
        (pid if q < B else nid)[q % B] = 1
    pid[[100, 101, 102, 103, 104]] = 2      # 5 positives + 4 negatives: heavy only by the sum
    nid[[7, 2000, 2001, 2002]] = 2
    pid[[200, 201, 202, 203]] = 3           # 4 + 4: walked, with both signs
    nid[[9, 300, 301, 2098]] = 3
    c = R.exact_case(rng, nu, ni, d, uid, pid, nid, m=0)
    cnt = _counts(c)
    assert cnt[nu + 1] == len(rel) and cnt[nu + 2] == 9 and cnt[nu + 3] == 8
    return c


@pytest.mark.parametrize("d", HEAVY_WIDTHS)
def test_item_rows_across_windows(dev, d):
    """B = 2,100: an item row, positives and negatives mixed, whose 10 hits in the scanned range
    [B, 3B) sit on both sides of a thread, a wave, the positive/negative and a window boundary
    and on the first and last position; an item heavy only by 5 positives plus 4 negatives; an
    item with 4 and 4, walked."""
    c = _item_window_case(d)
    _assert_exact(_backward(dev, c, what=f"item windows d = {d}"), c, f"item windows d = {d}")


@functools.lru_cache(maxsize=None)
def _makes_case(d):
    rng = np.random.default_rng(600 + d)
    nu, ni, B, keep = 200, 300, 701, 12
    uid, pid, nid = _background(rng, B, nu, ni, keep)
    _plant(rng, uid, [(0, 9), (1, 17), (2, 25), (3, 65), (4, 8)])
    _plant(rng, pid, [(0, 9), (1, 17), (2, 33), (3, 5), (4, 4)])
    _plant(rng, nid, [(3, 4), (4, 4), (5, 9), (6, 73)])
    same = np.flatnonzero((pid >= keep) & (nid >= keep))[:40]
    pid[same] = nid[same] = 11
    c = R.exact_case(rng, nu, ni, d, uid, pid, nid, m=1)
    cnt = _counts(c)
    assert cnt[:5].tolist() == [9, 17, 25, 65, 8]
    assert cnt[nu:nu + 7].tolist() == [9, 17, 33, 9, 8, 9, 73] and cnt[nu + 11] == 80
    assert c.coef[same].any() and not c.dE[nu + 11].any() and c.touched[nu + 11]
    return c


@pytest.mark.parametrize("d", [8] + HEAVY_WIDTHS)
def test_heavy_rows_of_every_make(dev, d):
    """Rows of exactly 9 hits (at d = 8 and 12 there are 256 lane groups, so most ranges of a
    window are empty), of 8k + 1 hits (17, 25, 33, 65, 73), an item heavy only by 5 positives
    plus 4 negatives, one with 4 + 4 (walked, mixed signs), and 40 batch rows with pid == nid:
    their item row is named 80 times and is exactly zero, as are those anchors' shares."""
    c, nu = _makes_case(d), 200
    dE = _backward(dev, c, what=f"heavy makes d = {d}")
    _assert_exact(dE, c, f"heavy makes d = {d}")
    assert not dE[nu + 11].any()


# ---- the heavy list ---------------------------------------------------------------------------
def _nines(rng, m, d):
    """B = 9m: m users, m positive items and m other negative items, each named 9 times."""
    B = 9 * m
    uid, pid, nid = (rng.permutation(np.repeat(np.arange(m), 9)) for _ in range(3))
    c = R.exact_case(rng, m + 3, 2 * m + 3, d, uid, pid, nid + m, m=0)
    cnt = _counts(c)
    assert B == c.B and (cnt[c.touched] == 9).all() and int(c.touched.sum()) == 3 * m
    return c


@pytest.mark.parametrize("d", HEAVY_WIDTHS)
def test_more_heavy_rows_than_blocks(dev, d):
    """B = 774: 86 users, 86 positive and 86 negative items of 9 positions each are 258 heavy
    rows for kHeavyGrid = 256 blocks, so two blocks take a second row. The list is also full:
    258 = 3B/9."""
    c = _nines(np.random.default_rng(774 + d), 86, d)
    assert c.B == 774 and int(c.touched.sum()) == 258
    _assert_exact(_backward(dev, c, what=f"258 heavy rows d = {d}"), c, f"258 heavy rows d = {d}")


@pytest.mark.parametrize("m", [1, 21, 100])
def test_heavy_list_filled_to_capacity(dev, m):
    """Every position in a row of exactly 9: 3m heavy rows, the capacity term 3B/9 of the list,
    in a workspace of exactly hgd_bpr_workspace_size bytes between guards. At m = 21 the list's
    64 slots end on the workspace's last byte."""
    for d in (16, 256):
        c = _nines(np.random.default_rng(m + d), m, d)
        assert 3 * c.B // 9 == 3 * m
        _assert_exact(_backward(dev, c, what=f"capacity m = {m}, d = {d}"), c,
                      f"capacity m = {m}, d = {d}")


# ---- index semantics --------------------------------------------------------------------------
def _edge_ids(n):
    return [-n - 1, -n, -1, 0, n - 1, n, 2 ** 62, -2 ** 62, I64_MIN, I64_MAX]


@functools.lru_cache(maxsize=None)
def _index_case(d):
    rng = np.random.default_rng(77 + d)
    nu, ni, B = 5, 7, 90
    uid, pid, nid = _background(rng, B, nu, ni, 0)
    uid[10:20], pid[30:40], nid[50:60] = _edge_ids(nu), _edge_ids(ni), _edge_ids(ni)
    uid[70], pid[70], nid[70] = nu, I64_MIN, -ni - 1     # three bad ids in one row
    uid[71], pid[71], nid[71] = -1, -1, -ni              # valid negatives
    uid[72], nid[72] = I64_MAX, I64_MAX
    c = R.exact_case(rng, nu, ni, d, uid, pid, nid, m=0)
    # 6 of the 10 edge ids are out of range; rows 70 and 72 count once each
    assert c.bad_rows == 3 * 6 + 2
    assert np.array_equal(c.pos[71], c.E[nu + ni - 1]) and np.array_equal(c.anc[71], c.E[nu - 1])
    assert np.array_equal(c.pos[32], c.E[nu + ni - 1])   # pid = -1: the last item, not a user
    return c


@pytest.mark.parametrize("d", [8, 60, 256])
def test_index_semantics(dev, d):
    """Negative ids wrap within their own block, out-of-range ones are clamped to the block's
    first or last row, and *bad_index rises by the number of batch ROWS holding one: the word
    starts at 3 and two calls leave 3 + 2·bad_rows. The table lies directly between guards."""
    c = _index_case(d)
    got = _forward(dev, c, bad0=3, calls=2, what=f"ids d = {d}")
    assert got.bad == 3 + 2 * c.bad_rows
    assert np.array_equal(bits(got.anc), bits(c.anc)) and np.array_equal(bits(got.pos), bits(c.pos))
    ref = R.forward(c.E, c.nu, c.ni, c.uid, c.pid, c.nid)
    assert np.abs(got.coef - ref.coef).max() <= 1e-5
    assert abs(got.loss - ref.loss) <= 1e-5 * np.mean(np.abs(ref.term) + 1)
    _assert_exact(_backward(dev, c, what=f"ids d = {d}"), c, f"ids d = {d}")


def test_a_clean_batch_leaves_the_word_alone(dev):
    c = _width_case(16)
    assert _forward(dev, c, bad0=41).bad == 41


def test_optional_outputs(dev):
    """bad_index, anc_out and pos_out may each be NULL, alone and together: the array behind a
    NULL keeps its sentinel (checked in _forward) and the other outputs are bitwise the same."""
    c = _index_case(60)
    full = _forward(dev, c)
    assert full.bad == c.bad_rows
    for anc, pos, bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1), (0, 0, 0)):
        got = _forward(dev, c, anc=bool(anc), pos=bool(pos), bad=bool(bad),
                       what=f"anc {anc} pos {pos} bad {bad}")
        assert np.array_equal(bits(got.coef), bits(full.coef))
        assert bits(np.array([got.loss]))[0] == bits(np.array([full.loss]))[0]
        if anc:
            assert np.array_equal(bits(got.anc), bits(full.anc))
        if pos:
            assert np.array_equal(bits(got.pos), bits(full.pos))
        if bad:
            assert got.bad == full.bad


# ---- forward values against float64 -----------------------------------------------------------
SCORES = [0.0, 10.0, -10.0, 20.0, -20.0, 88.0, -88.0, 200.0, -200.0]


@pytest.mark.parametrize("d", [4, 60, 252])
def test_forward_values(dev, d, capsys):
    """Random float tables, and rows engineered to the scores 0, ±10, ±20, ±88, ±200 (user 0 is
    the unit vector e_0, item j is s_j·e_0, the negative is a zero row: one exact product).
    Every coef and the loss are finite; |coef - ref| <= 1e-5 (the project's relative bound times
    |coef| < 1) and |loss - ref| <= 1e-5 · mean(|term| + 1) (the + 1 is the magnitude of
    1e-5 + sigmoid itself: near sigmoid -> 1 the term tends to -1e-5, and a bound relative to it
    would measure nothing). The largest error / bound of both is printed; on an MI355X it was
    1.3e-2, 1.3e-2 and 1.4e-2 for coef and 1.4e-3, 1.6e-3 and 4.2e-3 for the loss at d = 4, 60
    and 252."""
    rng = np.random.default_rng(d)
    nu, ni, B, n = 41, 53, 301, len(SCORES)
    E = (0.3 * rng.standard_normal((nu + ni, d))).astype(np.float32)
    E[0] = 0
    E[0, 0] = 1
    E[nu:nu + n + 1] = 0
    E[nu:nu + n, 0] = SCORES
    uid, pid, nid = rng.integers(1, nu, B), rng.integers(n + 1, ni, B), rng.integers(n + 1, ni, B)
    uid[:n], pid[:n], nid[:n] = 0, np.arange(n), n
    c = SimpleNamespace(E=E, nu=nu, ni=ni, d=d, B=B, uid=uid, pid=pid, nid=nid)
    ref = R.forward(E, nu, ni, uid, pid, nid)
    assert ref.s[:n].tolist() == SCORES and np.isfinite(ref.term).all()
    got = _forward(dev, c, what=f"values d = {d}")
    assert np.isfinite(got.coef).all() and np.isfinite(got.loss)
    assert np.array_equal(bits(got.anc), bits(E[uid])) and np.array_equal(bits(got.pos),
                                                                          bits(E[nu + pid]))
    coef_err = np.abs(got.coef - ref.coef)
    loss_bound = 1e-5 * np.mean(np.abs(ref.term) + 1)
    loss_err = abs(float(got.loss) - ref.loss)
    with capsys.disabled():
        print(f"\nbpr forward d = {d}: coef error / bound {coef_err.max() / 1e-5:.3e} (row "
              f"{int(coef_err.argmax())}, s = {ref.s[coef_err.argmax()]:.3f}), "
              f"loss error / bound {loss_err / loss_bound:.3e}")
    assert coef_err.max() <= 1e-5
    assert loss_err <= loss_bound


# ---- refusals on the device -------------------------------------------------------------------
def test_a_short_workspace_is_refused_and_nothing_is_written(dev):
    c = _index_case(8)
    need = _need(c)
    for fn, run in (("hgd_bpr_forward", _forward), ("hgd_bpr_backward", _backward)):
        status, message, outs = run(dev, c, short=1, what=fn)
        assert status == WORKSPACE
        assert message == f"{fn}: workspace {need - 1} < required {need}"
        for name, value in outs.items():
            if name == "bad":
                assert value.tolist() == [0]
            else:
                assert _is_sentinel(value), (fn, name)
