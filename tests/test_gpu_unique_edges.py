"""csrc/unique.hip at its constants: torch.unique(x.long()) through the three forms the package
offers — ``unique_long`` (range bitmap, radix sort beyond a 2^24 range), the raw device-complete
entry (``hgd_unique_dev_i64`` / ``hgd_unique_dev_trunc_f32``: window + far-key sort) and
``unique_long_n_group`` (the same kernels, blockIdx.y the list, then the clamp-and-zero tail) —
bit-exact against lists known by construction (tests/_unique_ref.py, checked against np.unique on
the CPU by tests/test_unique_ref.py). Every case names the guard it sits on.

Checked per form: ``unique_long`` — the list, and the attached ``_hgd_range`` = (min, max)
whenever the range fits the bitmap; raw entry — the count word, the list, and that nothing past
the count was written (the buffer is pre-filled; the raw entry has no tail pass); group — the
count, the list and a zero tail up to the capacity."""
import numpy as np
import pytest
import torch

from tests import _unique_ref as U

pytestmark = pytest.mark.gpu

GEOMETRY = U.geometry_cases()
FAR = U.far_cases()
FLOATS = U.float_cases()
FILL = -0x0123456789ABCDEF  # pre-fill of the raw entry's output: never a key of any case


def _raw(x, out=None, buf=None):
    """The single-list device-complete entry on caller-held buffers: (out, count tensor)."""
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    lib = nat.load()
    x = x.detach().contiguous().view(-1)
    n = x.numel()
    wsb = lib.hgd_unique_workspace_size(n)
    if out is None:
        out = torch.full((n,), FILL, dtype=torch.int64, device=x.device)
    if buf is None:
        buf = torch.empty(256 + wsb, dtype=torch.uint8, device=x.device)
    assert out.numel() >= n and buf.numel() >= 256 + wsb
    fn = lib.hgd_unique_dev_trunc_f32 if x.dtype == torch.float32 else lib.hgd_unique_dev_i64
    nat.check(fn(x.data_ptr(), n, out.data_ptr(), buf.data_ptr(), buf.data_ptr() + 256,
                 buf.numel() - 256, nat.stream_handle(x.device)), "hgd_unique_dev")
    return out, buf[:8].view(torch.int64)


def _check_raw(x, expected, out=None, buf=None):
    prefilled = out is None
    out, count = _raw(x, out, buf)
    k = int(count.item())
    assert k == len(expected), f"raw count {k} != {len(expected)}"
    assert U.same_list(out[:k], expected), "raw list"
    if prefilled:
        assert bool((out[k:] == FILL).all()), "raw entry wrote past the count"
    return out[:k]


def _check_group_entry(nodes, count, expected, cap):
    """One (nodes, count) of unique_long_n_group against the expected list cut to ``cap``."""
    live = min(len(expected), cap)
    assert nodes.dtype == torch.int64 and nodes.numel() == cap
    assert count.dtype == torch.int64 and int(count.item()) == live, "group count"
    assert U.same_list(nodes[:live], expected[:live]), "group list"
    assert not bool(nodes[live:].any()), "group tail not zero"


def _check_all(x, expected):
    from hypergraph_diffusion_for_recommendation_amd.functional import (unique_long,
                                                                         unique_long_n_group)
    expected = torch.as_tensor(expected).to(x.device)
    u = unique_long(x)
    assert U.same_list(u, expected), "unique_long list"
    lo, hi = int(expected[0]), int(expected[-1])
    if hi - lo < U.CAP_BITS:  # bitmap path: the range rides along
        assert u._hgd_range[:2] == (lo, hi)
    else:
        assert not hasattr(u, "_hgd_range")
    del u
    _check_raw(x, expected)
    (nodes, count), = unique_long_n_group([x])
    _check_group_entry(nodes, count, expected, x.numel())


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---------------------------------------------------------------- bitmap geometry
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_bitmap_geometry(dev, name):
    """Keys lo + bit for lo = -3 and 2^40 + 5. lastbitL: the span's last bit on a word
    (range_words' (span + 1 + 31) / 32) and on the 8-words-per-thread boundary (``w0 + j < words``
    in uq_count / uq_emit). words1023/1024/1025: the LDS bitmap against the global one (``words <=
    kLdsWords`` in uq_mark), keys in the first word, the last word and the words at the switch,
    more than one marking block. words2047 .. 4097: one, two and three tiles (kTileWords), bits
    65,535 / 65,536 and the last bit of the last tile; mid-empty: a tile whose offset stands
    still in uq_scan. window-sparse: span 2^24 - 1 (kCapBits), all kMaxTiles tiles. dense-tile:
    65,536 keys in one tile between one-key tiles (block_exclusive_scan, tile_off)."""
    keys, expected, _ = GEOMETRY[name]()
    _check_all(_t(keys, dev), expected)


@pytest.mark.parametrize("lo", U.LOS)
def test_full_window_dense(dev, lo):
    """Every bit of the 2^24-bit window set (kCapBits, kCapWords): n = 2^24 keys built on the
    device in descending order, every emit thread writes 256 keys, every tile counts 65,536
    (kTileWords · 32) and the one-block scan of uq_scan runs over all 256 tiles (kMaxTiles).
    Expected: dense()'s ascending run, no host sort."""
    n = U.CAP_BITS
    x = lo + (n - 1) - torch.arange(n, dtype=torch.int64, device=dev)
    small, small_exp = U.dense(lo, 64)
    assert np.array_equal(x[-64:].cpu().numpy(), small)  # the device build is dense()'s order
    expected = torch.arange(n, dtype=torch.int64, device=dev) + lo
    assert np.array_equal(expected[:64].cpu().numpy(), small_exp)
    _check_all(x, expected)


# ---------------------------------------------------------------- input size against the grids
@pytest.mark.parametrize("lo", U.LOS)
@pytest.mark.parametrize("n", U.SIZES)
def test_input_size_against_grids(dev, n, lo):
    """n on the 256-thread block and the 4,096 keys per min/max block; 131,072 / 131,073: the
    mark grid caps at kGrid · 256; 2,097,152 + 257: the min/max grid caps at kGrid · 4,096 and
    strides (``i += stride`` in uq_minmax / uq_mark). The minimum is the last element and the
    maximum the one before it: a grid short of the end loses the window."""
    keys, expected = U.sized_input(n, lo)
    _check_all(_t(keys, dev), expected)


# ---------------------------------------------------------------- window edge and far list
@pytest.mark.parametrize("name", list(FAR))
def test_window_edge_and_far_list(dev, name):
    """edge-*: a key at lo + 2^24 - 1 (inside: ``span >= kCapBits`` false) and at lo + 2^24 (the
    first far key: ``b >= kCapBits`` in uq_mark). farK-single: exactly K far entries — the LDS
    sort against the workspace bitonic (``P <= kFarLds``), K a power of two and next to one
    (``while (P < k)``), the 1,024-wide chunks of the distinct pass (kFarThreads).
    farK-copies: 1 to 3 copies per key, runs of equal keys over sorted positions 1,023/1,024 and
    4,095/4,096 (the ``prev`` read at a chunk start). far-all-equal: one run. far-int64-max-*:
    a real key equal to the LLONG_MAX pad, k not a power of two, in LDS and in the workspace.
    lo-int64-min*: ``key - lo`` and ``hi - lo`` in unsigned arithmetic. ``unique_long`` takes
    its radix-sort path on the same inputs and must agree."""
    keys, expected, _ = FAR[name]()
    _check_all(_t(keys, dev), expected)


@pytest.mark.parametrize("name", list(FLOATS))
def test_float_sources(dev, name):
    """TruncSrc: truncation toward zero (±0.999, ±0.0 one key, denormals), 2^24 - 1 inside the
    window and 2^24 the first far key, ±(2^63 - 2^39) the last floats in range, and 2^63,
    -2^63 - 2^40, NaN, ±inf → INT64_MIN (``!(fabsf(x) < 2^63)``); lds-switch: the LDS / global
    bitmap switch from a float source. Expected: np.unique of trunc_long."""
    x, _ = FLOATS[name]
    expected = U.unique_ref(U.trunc_long(x))
    _check_all(_t(x, dev), expected)


# ---------------------------------------------------------------- groups
def _group_lists(dev):
    """Five (tensor, expected) lists of different kinds for the group tests."""
    g = [GEOMETRY["words1025-lo0"]()[:2], FAR["far1025-copies"]()[:2],
         U.sized_input(257, U.LOS[1]), GEOMETRY["lastbit256-lo40"]()[:2],
         FAR["far-int64-max-lds"]()[:2]]
    out = [(_t(k, dev), e) for k, e in g]
    x, _ = FLOATS["indefinite-and-others"]
    out.append((_t(x, dev), U.unique_ref(U.trunc_long(x))))
    return out


def _check_group(xs, expecteds, n_rows=None, caps=None):
    """``caps``: the capacity each list must come back with, written out by the test (not the
    wrapper's formula); without ``n_rows`` it is the list's length."""
    from hypergraph_diffusion_for_recommendation_amd.functional import unique_long_n_group
    assert (n_rows is None) == (caps is None)
    got = unique_long_n_group(xs, n_rows)
    assert len(got) == len(xs)
    for k, (x, e) in enumerate(zip(xs, expecteds)):
        cap = x.numel() if caps is None else caps[k]
        _check_group_entry(got[k][0], got[k][1], e, cap)
        single = _check_raw(x, e)  # and the single-list entry gives the same list
        live = min(len(e), cap)
        assert torch.equal(got[k][0][:live], single[:live]), k
    return got


@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 6])
def test_group_list_counts(dev, count):
    """1 to 4 lists in one launch (kMaxJobs, blockIdx.y picks the job), 5 and 6 spill into a
    second launch; bitmap, far-LDS, far-workspace and float lists side by side, each equal to
    the single-list entry's result."""
    lists = _group_lists(dev)[:count]
    _check_group([x for x, _ in lists], [e for _, e in lists])


def test_group_mixed_sizes(dev):
    """n = 1, 257 and 2,097,409 in one group: the grids are sized for n_max, so the small lists
    ride a kGrid-block grid (blocks past a list's end must neither mark nor disturb min/max),
    and k_uqg_tail strides over the largest."""
    sizes = (1, 257, 2097152 + 257)
    pairs = [U.sized_input(n, lo) for n, lo in zip(sizes, (7, U.LOS[0], U.LOS[1]))]
    _check_group([_t(k, dev) for k, _ in pairs], [e for _, e in pairs])
    _check_group([_t(k, dev) for k, _ in pairs[::-1]], [e for _, e in pairs[::-1]])


def test_group_far_between_near(dev):
    """A far-list job between two jobs without far keys: State::far_n and the far buffer are per
    job (``if (kk == 0) return`` must hold for the neighbours), in LDS and in the workspace."""
    for far in ("far1024-copies", "far4097-single"):
        pairs = [GEOMETRY["words1024-lo40"]()[:2], FAR[far]()[:2], GEOMETRY["lastbit31-lo0"]()[:2]]
        _check_group([_t(k, dev) for k, _ in pairs], [e for _, e in pairs])


def test_group_float_next_to_int64(dev):
    """AnySrc: the same keys as a float32 list and as an int64 list in one launch."""
    x, _ = FLOATS["lds-switch"]
    keys = U.trunc_long(x)
    e = U.unique_ref(keys)
    y, _ = FLOATS["indefinite-and-others"]
    ky = U.trunc_long(y)
    _check_group([_t(x, dev), _t(keys, dev), _t(ky, dev), _t(y, dev)],
                 [e, e, U.unique_ref(ky), U.unique_ref(ky)])


def test_group_capacity(dev):
    """k_uqg_tail: ``capacity`` = min(n, 2·n_rows) exactly the count, count - 1, 1 and above the
    count — the count is clamped, the kept prefix is the smallest keys, out[count, capacity) is
    zero; and a cut that falls inside the far part of the output (the ``pos < n`` side of
    uq_far stays the list's n, the tail pass trims)."""
    even = U.bits_at(-3, [0, 2, 3, 40, 300, 70000], 5, seed=1)          # 6 distinct, n = 30
    odd = U.bits_at(U.LOS[1], [0, 1, 31, 32, 33, 2000, 70000], 5, seed=2)  # 7 distinct, n = 35
    far = U.with_far(U.bits_at(-3, [0, 1, 2], 4), U.far_keys(-3, 6, (2, 1, 3)))  # 3 + 6, n = 24
    cases = ((even, [3, 2, 0, 100], [6, 4, 1, 30]),   # the count, below it, 1, n (above it)
             (odd, [3, 0, 100, 4], [6, 1, 35, 8]),    # count - 1, 1, n, above the count
             (far, [3, 2, 1, 4], [6, 4, 2, 8]))       # 3 near + 3 of 6 far, near only, 8 of 9
    assert [len(c[0][0]) for c in cases] == [30, 35, 24]  # n: the capacity never exceeds it
    for (keys, e), rows, caps in cases:
        _check_group([_t(keys, dev)] * len(rows), [e] * len(rows), rows, caps)
    assert len(even[1]) == 6 and len(odd[1]) == 7 and len(far[1]) == 9  # = 2·3, 2·3 + 1, 3 + 6


# ---------------------------------------------------------------- workspace reuse
def test_workspace_reuse(dev):
    """One caller-held workspace and output through the raw entry, three calls in a row: a full
    2^24 window, a 5-bit range, a far-list input. uq_zero clears only the words of the current
    range, uq_count writes only the current tiles and uq_init resets far_n: the later calls must
    see nothing of the full bitmap, the 256 tile counts or an earlier far list."""
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    lo = U.LOS[1]
    n = U.CAP_BITS
    wsb = nat.load().hgd_unique_workspace_size(n)
    buf = torch.empty(256 + wsb, dtype=torch.uint8, device=dev)
    out = torch.empty(n, dtype=torch.int64, device=dev)
    x = lo + (n - 1) - torch.arange(n, dtype=torch.int64, device=dev)
    _check_raw(x, torch.arange(n, dtype=torch.int64, device=dev) + lo, out, buf)
    five = U.bits_at(lo + 3, [0, 1, 2, 3, 4], 100, seed=3)
    far = FAR["far4097-copies"]()[:2]
    again = U.bits_at(lo, [0, 4, U.TILE_BITS + 1], 3, seed=4)
    for keys, e in (five, far, again, far, five):
        _check_raw(_t(keys, dev), e, out, buf)


def test_same_call_twice_and_on_a_side_stream(dev):
    """The same call twice on the current stream and once on a side stream that waited for it,
    on one workspace: all three results are equal (no state survives a call, every kernel runs
    on the stream it is given)."""
    keys, e = FAR["far1025-copies"]()[:2]
    x = _t(keys, dev)
    from hypergraph_diffusion_for_recommendation_amd import _native as nat
    wsb = nat.load().hgd_unique_workspace_size(x.numel())
    buf = torch.empty(256 + wsb, dtype=torch.uint8, device=dev)
    outs = [torch.full((x.numel(),), FILL, dtype=torch.int64, device=dev) for _ in range(3)]
    counts = []
    for o in outs[:2]:
        counts.append(_raw(x, o, buf)[1].clone())
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        counts.append(_raw(x, outs[2], buf)[1].clone())
    side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    for o, c in zip(outs, counts):
        assert int(c.item()) == len(e)
        assert U.same_list(o[:len(e)], e) and bool((o[len(e):] == FILL).all())
        assert torch.equal(o, outs[0])
