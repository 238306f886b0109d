"""Chunk and workgroup boundaries of the block primitives (csrc/cs_block.h: block_scan_incl, block_rank, uf_find / uf_unite)
through the kernels that use them.  Every result is an integer and every comparison is exact, against numpy or the restatements in
tests/ (detect_ref, regions_ref, the top-k oracle of test_pool_head_topk_gpu)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detect_ref  # noqa: E402
import regions_ref  # noqa: E402
from test_pool_head_topk_gpu import _run_topk, _sample_reference  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402

pytestmark = pytest.mark.gpu

T_SECOND_PASS = 257 * 2048 + 1        # 258 blocks of 2048 positions: the block-count scan takes a second pass, the last block holds 1 item


# ---- topk.hip: sel_scan_kernel / sel_write_kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 7, 8, 9, 2047, 2048, 2049, 4097, T_SECOND_PASS])
def test_threshold_select_chunk_edges(T, dev):
    rs = np.random.RandomState(T % 1000)
    probs = rs.rand(T).astype(np.float32)
    probs[rs.rand(T) < 0.3] = 0.5                      # ties exactly on the middle threshold
    order = rs.permutation(T).astype(np.int64)         # independent of the sorter
    pd, od = torch.from_numpy(probs).to(dev), torch.from_numpy(order).to(dev)
    for thr in (-1.0, 0.5, 2.0):                       # everything, a tie-laden cut, nothing
        out, cnt = K.threshold_select(pd, od, thr)
        want = order[probs[order] > np.float32(thr)]
        n = int(cnt.cpu())
        assert n == len(want), (T, thr)
        assert np.array_equal(out[:n].cpu().numpy(), want), (T, thr)


def test_segmented_topk_second_scan_pass(dev):
    rs = np.random.RandomState(7)
    sizes = []
    while sum(sizes) < T_SECOND_PASS:                  # runs of at most 8192 tiles: the LDS sorter
        sizes.append(min(int(rs.randint(1, 8193)), T_SECOND_PASS - sum(sizes)))
    groups = np.repeat(np.arange(len(sizes)), sizes)
    labels = {g: int(rs.choice([0, 0, 1, 2, 5, 40])) for g in range(len(sizes))}
    probs = rs.rand(T_SECOND_PASS).astype(np.float32)
    probs[rs.rand(T_SECOND_PASS) < 0.3] = 0.5
    got = _run_topk(probs, groups, labels, 3, 30, dev)
    assert np.array_equal(got, _sample_reference(probs, groups, labels, 3, 30))


# ---- topk.hip: prune_kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 6145])
def test_prune_excess_chunk_edges(n, flag, dev):
    labels = np.random.RandomState(n).randint(0, 2, size=n).astype(np.int32)
    ld = torch.from_numpy(labels).to(dev)
    flagged = np.flatnonzero(labels == flag)
    on_edge = int((labels[:2048] == flag).sum())       # the cut falls exactly on the end of the first chunk
    for n_excess in dict.fromkeys([0, 1, on_edge, len(flagged), len(flagged) + 5]):
        kept, cnt = K.prune_excess(ld, flag, n_excess)
        want = np.setdiff1d(np.arange(n), flagged[:n_excess])
        m = int(cnt.cpu())
        assert m == len(want), (n, flag, n_excess)
        assert np.array_equal(kept[:m].cpu().numpy(), want), (n, flag, n_excess)


# ---- detect.hip: cluster_offsets_kernel, cluster_ids_kernel, both clustering paths ---------------------------------------------------
def _assert_clusters(pts, n_pts, eps, weights, want, force_global, dev):
    """pts int32 [N, cap, 2], n_pts [N]; want: per map (points, weights) of detect_ref.cluster"""
    N = len(n_pts)
    bl = torch.from_numpy(weights).to(dev)[None].expand(N, -1, -1).contiguous()
    out_pts, out_w, off = K.detect_cluster(torch.from_numpy(pts).to(dev), torch.from_numpy(n_pts).to(dev), eps, bl, force_global=force_global)
    off, out_pts, out_w = off.cpu().numpy(), out_pts.cpu().numpy(), out_w.cpu().numpy()
    assert np.array_equal(off, np.r_[0, np.cumsum([len(w) for _, w in want])])
    assert np.array_equal(out_pts[:off[-1]], np.concatenate([p for p, _ in want]))
    assert np.array_equal(out_w[:off[-1]], np.concatenate([w for _, w in want]))


@functools.lru_cache(maxsize=None)
def _many_maps(N):
    rng = np.random.RandomState(N)
    weights = rng.randint(0, 4, size=(32, 32)).astype(np.uint8)          # few levels: ties, so the label order matters
    pts = rng.randint(0, 32, size=(N, 8, 2)).astype(np.int32)
    n_pts = (np.arange(N) % 9).astype(np.int32)                          # 0..8 points: empty maps at the chunk edges too
    want = tuple(detect_ref.cluster(pts[i, :n_pts[i]], 3.0, weights) for i in range(N))
    return pts, n_pts, weights, want


@pytest.mark.parametrize("force_global", [False, True])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
def test_cluster_offsets_across_256_maps(N, force_global, dev):
    pts, n_pts, weights, want = _many_maps(N)
    _assert_clusters(pts, n_pts, 3.0, weights, want, force_global, dev)


@functools.lru_cache(maxsize=None)
def _one_map(n):
    rng = np.random.RandomState(n)
    weights = rng.randint(0, 4, size=(299, 299)).astype(np.uint8)
    pts = rng.randint(0, 299, size=(1, n, 2)).astype(np.int32)
    return pts, np.array([n], np.int32), weights, (detect_ref.cluster(pts[0], 11.0, weights),)


@pytest.mark.parametrize("force_global", [False, True])
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2048, 2049])            # 2049 points leave the LDS path on their own
def test_cluster_numbering_across_1024_points(n, force_global, dev):
    pts, n_pts, weights, want = _one_map(n)
    _assert_clusters(pts, n_pts, 11.0, weights, want, force_global, dev)


# ---- regions.hip: number_count / number_scan / number_assign, tile and border unions ---------------------------------------------------
@pytest.mark.parametrize("thinned", [False, True])
@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("hw", [(1, 1024), (1, 1025), (1024, 1024), (1025, 1024)])       # 1, 2, 1024, 1025 blocks of 1024 pixels per image
def test_label_numbering_block_edges(hw, connectivity, thinned, dev):
    H, W = hw
    mask = np.zeros((2, H, W), bool)
    mask[:, 0::2, 0::3] = True                         # no two foreground pixels touch, even diagonally: one component per pixel
    if thinned:
        mask &= np.random.RandomState(H + W).rand(2, H, W) >= 0.3
    want = np.stack([np.cumsum(m.ravel()).reshape(H, W) * m for m in mask]).astype(np.int32)          # scipy numbers in raster order
    got = K.regions_label(torch.from_numpy(mask.astype(np.uint8)).to(dev), connectivity)
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("connectivity", [1, 2])
def test_label_blobs_across_tiles(connectivity, dev):
    mask = regions_ref.blobs(1, 130, 97, seed=5)
    got = K.regions_label(torch.from_numpy(mask.astype(np.uint8)).to(dev), connectivity)
    assert np.array_equal(got[0].cpu().numpy(), regions_ref.label(mask[0], connectivity)[0])
