"""CPU-only: the numpy model of the scan segmentation (tests/segment_common.py) against an independent labelling — on the
mask-drawn scenes scipy.ndimage.label with a merge across the seam must give the mask's components plus the complement's — and
the preconditions the GPU tests rest on: the real scenes must hold enough accepted and rejected components and a sane ground
share, so that no GPU test passes on an empty graph."""
import numpy as np
import pytest
from scipy import ndimage

import segment_common as M
from loam_amd import capi

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])


def labelled(mask):
    """4-connected components of a cylindrical mask: ndimage.label, then the labels that meet across the seam are merged.
    Returns per cell the smallest linear index of its component, -1 outside the mask."""
    H, W = mask.shape
    lab, n = ndimage.label(mask, structure=CROSS)
    parent = np.arange(n + 1)

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    if W > 1:
        for l in np.flatnonzero(mask[:, 0] & mask[:, -1]):
            a, b = find(lab[l, 0]), find(lab[l, -1])
            parent[max(a, b)] = min(a, b)
    comp = np.array([find(x) for x in range(n + 1)])[lab]
    root = np.full((H, W), -1, np.int64)
    idx = np.arange(H * W).reshape(H, W)
    for c in np.unique(comp[mask]):
        sel = mask & (comp == c)
        root[sel] = idx[sel].min()
    return root


@pytest.mark.parametrize("H,W", [(8, 37), (19, 300), (5, 16), (1, 16), (21, 556)])
def test_mask_scenes_give_the_masks_components_plus_the_complements(H, W):
    params = capi.SegmentParams(**M.MASK_PARAMS)
    masks = [M.random_mask(H, W, s) for s in (1, 2, 3)] + [M.serpentine(H, W), M.comb(H, W), M.alternating_lines(H, W), M.checkerboard(H, W),
                                                           np.ones((H, W), bool), np.zeros((H, W), bool)]
    for k, mask in enumerate(masks):
        for far in (20.0, None):
            seg = M.segment(M.mask_scan(mask, far=far), H, W, params=params)
            assert seg.stats[1] == 0, "something is ground on a sphere about the sensor"
            want = labelled(mask)
            if far is not None:
                other = labelled(~mask)
                want = np.where(mask, want, other)
            want = np.where(want < 0, M.NO_LABEL, want).astype(np.uint32).reshape(-1)
            assert np.array_equal(seg.labels, want), (H, W, k, far)
            assert np.array_equal(seg.sizes, np.where(want == M.NO_LABEL, 0, np.bincount(want[want != M.NO_LABEL], minlength=H * W)[np.minimum(want, H * W - 1)]))
            assert seg.stats[0] == (0 if far is not None else int((~mask).sum()))


@pytest.mark.parametrize("name", ("canyon", "lot", "field"))
def test_real_scenes_hold_what_the_gpu_tests_need(name):
    H, W = 32, 512
    seg = M.segment(M.real_scan(name), H, W)
    accepted, rejected, ground_share = int(seg.stats[4]), int(seg.stats[5]), seg.stats[1] / (H * W)
    assert accepted >= 50 and rejected >= 20 and 0.3 < ground_share < 0.95, (name, accepted, rejected, ground_share)
    assert int(seg.stats[:4].sum()) == H * W and seg.stats[2] + seg.stats[3] == np.count_nonzero(seg.labels != M.NO_LABEL)
    assert len(seg.clusters) == accepted and (np.diff(seg.clusters["root"].astype(np.int64)) > 0).all()
    assert int(seg.clusters["size"].sum()) == seg.stats[2]
    # the filtered scan: dropped cells are +0, kept cells are the input's bits
    keep = (seg.classes == capi.SEGMENT_CLUSTER) | (seg.classes == capi.SEGMENT_GROUND)
    scan = M.real_scan(name)
    assert np.array_equal(seg.filtered[keep].view(np.uint64), scan[keep].view(np.uint64)) and not seg.filtered[~keep].view(np.uint64).any()


def test_census_model_counts_border_edges_only_in_the_tile_form():
    H, W = 21, 556
    seg = M.segment(M.mask_scan(M.serpentine(H, W)), H, W, params=capi.SegmentParams(**M.MASK_PARAMS))
    every, border = M.merged_edges(seg, 16, 256, False), M.merged_edges(seg, 16, 256, True)
    assert every == int(seg.right.sum() + seg.up.sum()) and 0 < border < every
    assert M.merged_edges(seg, H, W, True) == int(seg.right[:, -1].sum() + seg.up[-1].sum())  # one tile: only the seam
