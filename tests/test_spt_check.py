"""spt_check.assert_same is the comparison every smallpt GPU test goes
through: it must fail on a single differing bit in any field, compare colours
as bit patterns, and read both frame classes."""
import types

import numpy as np
import pytest

import spt_check


def _frame(seed=3, n=24):
    rng = np.random.default_rng(seed)
    col = rng.standard_normal(3 * n).astype(np.float32)
    seeds = rng.integers(2, 1 << 32, 2 * n, dtype=np.uint64).astype(np.uint32)
    px = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return col, seeds, px, (11, 22, 33, 44)


def _flip(arr, slot, bit):
    out = arr.copy()
    out.view(np.uint32)[slot] ^= np.uint32(1 << bit)
    return out


def test_identical_tuples_pass():
    ref = _frame()
    spt_check.assert_same(tuple(np.copy(a) for a in ref[:3]) + (ref[3],), ref)
    spt_check.assert_same(ref[:3], ref)                  # no counters on one side: the rest still compared
    spt_check.assert_same(ref, ref[:3])
    spt_check.assert_same(ref, ref, counted=True)


@pytest.mark.parametrize("field", [0, 1, 2])
@pytest.mark.parametrize("slot,bit", [(0, 0), (7, 31), (-1, 12)])
def test_one_flipped_bit_fails(field, slot, bit):
    ref = _frame()
    got = list(ref)
    got[field] = _flip(ref[field], slot, bit)
    for counted in (None, False, True):
        with pytest.raises(AssertionError):
            spt_check.assert_same(tuple(got), ref, counted=counted)
        if counted is not True:
            with pytest.raises(AssertionError):
                spt_check.assert_same(tuple(got[:3]), ref[:3], counted=counted)


@pytest.mark.parametrize("k", range(4))
def test_one_counter_bit_fails(k):
    ref = _frame()
    cnt = list(ref[3])
    cnt[k] ^= 1
    got = ref[:3] + (tuple(cnt),)
    with pytest.raises(AssertionError):
        spt_check.assert_same(got, ref)
    with pytest.raises(AssertionError):
        spt_check.assert_same(got, ref, counted=True)
    spt_check.assert_same(got, ref, counted=False)       # an uncounted launch: counters not compared
    with pytest.raises(AssertionError):
        spt_check.assert_same(ref[:3], ref, counted=True)   # counted=True needs counters on both sides


def test_colours_compare_as_bit_patterns():
    ref = _frame()
    nan = ref[0].copy()
    nan.view(np.uint32)[5] = 0x7FC00001
    spt_check.assert_same((nan,) + ref[1:], (nan.copy(),) + ref[1:])     # the same NaN: equal
    other = nan.copy()
    other.view(np.uint32)[5] = 0x7FC00002                                # another NaN payload
    with pytest.raises(AssertionError):
        spt_check.assert_same((other,) + ref[1:], (nan,) + ref[1:])
    with pytest.raises(AssertionError):
        spt_check.assert_same((nan,) + ref[1:], ref)                     # NaN against a number
    pz, nz = ref[0].copy(), ref[0].copy()
    pz[9], nz[9] = 0.0, -0.0
    assert pz[9] == nz[9]
    with pytest.raises(AssertionError):
        spt_check.assert_same((pz,) + ref[1:], (nz,) + ref[1:])


def _host_frame(ref):
    """rtamd.SmallptFrame's attributes: numpy arrays and a counter list."""
    return types.SimpleNamespace(colors=ref[0], seeds=ref[1], pixels=ref[2], counters=list(ref[3]))


def _device_frame(ref):
    """rtamd.SmallptDeviceFrame's: host() and a counter tensor (tolist())."""
    return types.SimpleNamespace(host=lambda: ref[:3], counters=np.array(ref[3], np.int64))


@pytest.mark.parametrize("make", [_host_frame, _device_frame])
def test_both_frame_classes(make):
    ref = _frame()
    spt_check.assert_same(make(ref), ref)
    spt_check.assert_same(make(ref), make(ref), counted=True)
    for field in range(3):
        bad = list(ref)
        bad[field] = _flip(ref[field], 2, 3)
        with pytest.raises(AssertionError):
            spt_check.assert_same(make(tuple(bad)), ref)
    with pytest.raises(AssertionError):
        spt_check.assert_same(make(ref[:3] + ((11, 22, 33, 45),)), ref)
    spt_check.assert_same(make(ref[:3] + ((0, 0, 0, 0),)), ref, counted=False)


def test_oracle_frame_is_read_only_and_progressive(oracle):
    ref = spt_check.oracle_frame(oracle, 16, 8, [1, 2])
    for a in ref[:3]:
        assert not a.flags.writeable
    assert isinstance(ref[3], tuple) and len(ref[3]) == 4 and ref[3][3] == 16 * 8 * 3
    spt_check.assert_same(spt_check.oracle_frame(oracle, 16, 8, [3], nthreads=1), ref, counted=True)
    get = spt_check.frame_cache(oracle)
    assert get(16, 8, [1, 2]) is get(16, 8, (1, 2))
    spt_check.assert_same(get(16, 8, [1, 2]), ref, counted=True)
    win = get(16, 8, [3], rows=(2, 5))
    inside = np.zeros((8, 16), bool)
    inside[8 - 5:8 - 2] = True                       # accumulator rows are flipped
    ins = inside.reshape(-1)
    assert (win[0].reshape(-1, 3)[ins].view(np.uint32) == ref[0].reshape(-1, 3)[ins].view(np.uint32)).all()
    assert not win[0].reshape(-1, 3)[~ins].any()
