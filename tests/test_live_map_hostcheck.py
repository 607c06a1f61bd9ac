"""CPU-only: xcd_map.h — xcd_live_map, by which the kernels of ICF iterations 3+ deal the pairs that still run over the 8 XCD
lanes (loam_amd/csrc/register_kernels.hip: assoc_map), and xcd_pair_map, the placement of every pair — compiled with g++
(tests/hostcheck_live) and walked workgroup by workgroup: whole grids (ceil(n_pairs / 8) * 8 * blocks_per_pair workgroups,
what launch_associate sizes them to) and a stretch past their end."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "hostcheck_live")
NONE = 0xFFFFFFFF
BLOCKS_PER_PAIR = (1, 2, 5, 77)
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", DIR])
        _lib = C.CDLL(os.path.join(DIR, "libhostcheck_live.so"))
    return _lib


def grid_blocks(n_pairs, bpp):
    return (n_pairs + 7) // 8 * 8 * bpp


def _walk(fn, n_blocks, *args):
    ok, pair, chunk = np.zeros(n_blocks, np.uint8), np.zeros(n_blocks, np.uint32), np.zeros(n_blocks, np.uint32)
    u32p = C.POINTER(C.c_uint32)
    fn(C.c_uint32(n_blocks), *args, ok.ctypes.data_as(C.POINTER(C.c_uint8)), pair.ctypes.data_as(u32p), chunk.ctypes.data_as(u32p))
    return ok.astype(bool), pair, chunk


def live_walk(n_pairs, bpp, live, extra=0):
    live = np.ascontiguousarray(live, dtype=np.uint32)
    buf = np.concatenate([live, np.full(3, NONE, np.uint32)])  # (what lies past the list is no pair: it must not be read as one)
    return _walk(lib().hostcheck_live_walk, grid_blocks(n_pairs, bpp) + extra, C.c_uint32(bpp), C.c_uint64(n_pairs), C.c_uint32(len(live)),
                 buf.ctypes.data_as(C.POINTER(C.c_uint32)))


def pair_walk(n_pairs, bpp, extra=0):
    return _walk(lib().hostcheck_pair_walk, grid_blocks(n_pairs, bpp) + extra, C.c_uint32(bpp), C.c_uint64(n_pairs))


def check_deal(n_pairs, bpp, live):
    """every property the kernels rely on, for one list"""
    live = np.asarray(live, dtype=np.uint32)
    n_live, grid = len(live), grid_blocks(n_pairs, bpp)
    ok, pair, chunk = live_walk(n_pairs, bpp, live, extra=16 * bpp)
    tag = (n_pairs, bpp, live.tolist())
    # every (live pair, chunk) by exactly one workgroup, nothing else by any
    got = np.sort(pair[ok].astype(np.int64) * bpp + chunk[ok])
    want = np.sort((live.astype(np.int64)[:, None] * bpp + np.arange(bpp)[None, :]).ravel())
    assert np.array_equal(got, want), tag
    assert (chunk[ok] < bpp).all(), tag
    dead = np.setdiff1d(np.arange(n_pairs), live)
    assert not np.isin(pair[ok], dead).any(), tag
    # workgroups past the live range have nothing to do — inside the grid and past its end
    block = np.arange(len(ok))
    idx = (block & 7) + 8 * ((block >> 3) // bpp)
    assert np.array_equal(ok, idx < n_live), tag
    assert not ok[grid:].any(), tag
    # all chunks of a pair on one XCD lane; the lanes' pair counts differ by one at most
    lane_of = np.full(n_pairs, -1, np.int64)
    lanes = block[ok] & 7
    for p, l in zip(pair[ok], lanes):
        assert lane_of[p] in (-1, l), tag
        lane_of[p] = l
    counts = np.bincount(lane_of[live], minlength=8) if n_live else np.zeros(8, np.int64)
    assert counts.sum() == n_live and counts.max() - counts.min() <= 1, tag


@pytest.mark.parametrize("bpp", BLOCKS_PER_PAIR)
def test_every_live_subset_of_the_small_batches(bpp):
    rng = np.random.default_rng(11)
    for n_pairs in (8, 9, 10):
        for mask in itertools.product((False, True), repeat=n_pairs):
            live = np.flatnonzero(mask).astype(np.uint32)
            rng.shuffle(live)  # (order inside the list is free)
            check_deal(n_pairs, bpp, live)


@pytest.mark.parametrize("bpp", BLOCKS_PER_PAIR)
def test_random_live_subsets_of_batches_up_to_40_pairs(bpp):
    rng = np.random.default_rng(12)
    for n_pairs in range(11, 41):
        sizes = {0, 1, 7, 8, 9, n_pairs - 1, n_pairs} | set(rng.integers(0, n_pairs + 1, 12).tolist())
        for n_live in sorted(sizes):
            check_deal(n_pairs, bpp, rng.permutation(n_pairs)[:n_live])


@pytest.mark.parametrize("bpp", BLOCKS_PER_PAIR)
def test_the_full_list_in_pair_order_is_the_pair_map(bpp):
    for n_pairs in range(8, 41):
        a = live_walk(n_pairs, bpp, np.arange(n_pairs), extra=16 * bpp)
        b = pair_walk(n_pairs, bpp, extra=16 * bpp)
        for x, y in zip(a, b):
            assert np.array_equal(x, y), (n_pairs, bpp)
        # ... which gives every pair's every chunk once, pair p on lane p % 8
        ok, pair, chunk = b
        assert np.array_equal(np.sort(pair[ok].astype(np.int64) * bpp + chunk[ok]), np.arange(n_pairs * bpp))
        assert np.array_equal(np.flatnonzero(ok) & 7, pair[ok] & 7)


def test_a_list_entry_that_is_no_pair_gives_no_work():
    # (nothing writes such an entry; a workgroup that met one must leave, not index the batch with it)
    ok, pair, _ = live_walk(16, 3, [3, 16, NONE, 5])
    assert sorted(set(pair[ok].tolist())) == [3, 5] and ok.sum() == 6


def test_the_same_walk_is_clean_under_asan_and_ubsan_in_a_stand_alone_program():
    subprocess.check_call(["make", "-s", "-C", DIR, "san"])
    out = subprocess.run([os.path.join(DIR, "hostcheck_live_san")], capture_output=True, text=True, timeout=300)
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "hostcheck_live ok" in out.stdout, text[-3000:]
    assert "runtime error" not in text and "AddressSanitizer" not in text, text[-3000:]
