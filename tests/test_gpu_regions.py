"""Merging regions by similarity on the MI355X (fast_slic_amd/regions.py, csrc/region.hip) against the model written from the rules
(tests/region_ref.py), with exact equality throughout: group sums bit for bit against the exact sum of tests/pool_ref.py (node counts
around a block of 256, one accumulator taking every add, values that cancel across 120 binary orders), edge weights bit for bit
against numpy float32 arithmetic (edge counts around a block, and once round the kernel's loop), limit_joins against the sorted keys,
and merge_hierarchical against the model's rounds, against a re-pool of the relabelled pixels and against the graph of the relabelled
map."""
import functools

import numpy as np
import pytest
import torch

import merge_ref as M
import rag_ref
import region_ref as R
from fast_slic_amd.merge import best_neighbour_edges, merge_components, merge_labels
from fast_slic_amd.pool import superpixel_pool
from fast_slic_amd.rag import superpixel_graph
from fast_slic_amd.regions import MergeResult, edge_weights, group_sums, limit_joins, merge_hierarchical
from test_gpu_merge import map_case, same, to_dict, to_graph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- group_sums ----
def spread_values(rng, shape, lo=-20, hi=20):
    """Normal float32 values of either sign with 24 random mantissa bits and exponents spread over [lo, hi]."""
    return (np.ldexp(rng.integers(1 << 23, 1 << 24, shape).astype(np.float64), rng.integers(lo, hi + 1, shape) - 23)
            * rng.choice([-1.0, 1.0], shape)).astype(F32)


def check_sums(values, mapping, K2, counts=None):
    want = R.group_sums(values, mapping, K2, counts)
    got = group_sums(dev(values), dev(mapping), K2, None if counts is None else dev(counts))
    N, Cc = mapping.shape[0], values.shape[-2]
    if counts is not None:
        (want, want_c), (got, got_c) = want, got
        assert got_c.dtype == dev(counts).dtype and tuple(got_c.shape) == (N, K2) and got_c.device == DEV
        assert np.array_equal(got_c.cpu().numpy(), want_c)
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, Cc, K2) and got.device == DEV
    assert np.array_equal(bits(got), bits(want))
    return got


@pytest.mark.parametrize("K", [1, 255, 256, 257, 1600])
def test_sums_around_a_block(K):
    rng = np.random.default_rng(K)
    for N in (1, 3):
        for Cc in (1, 3, 17):
            K2 = max(K // 3, 1)
            values = spread_values(rng, (N, Cc, K))
            mapping = rng.integers(-1, K2 + 2, (N, K)).astype(np.int32)    # -1, K2 and K2 + 1 add nothing
            counts = rng.integers(0, 1000, (N, K)).astype(np.int32 if Cc == 3 else np.int64)
            check_sums(values, mapping, K2, counts if Cc > 1 else None)
    one = check_sums(values[0], mapping[:1], K2, counts[0])               # [C, K] values and [K] counts with N = 1
    assert tuple(one.shape) == (1, 17, K2)


def test_sums_of_the_most_nodes():
    K = 65534
    rng = np.random.default_rng(5)
    values = spread_values(rng, (1, 1, K))
    mapping = rng.integers(-1, K + 1, (1, K)).astype(np.int32)
    mapping[0, :2] = (K - 1, K)                                            # the last group, and a number next to it
    check_sums(values, mapping, K, rng.integers(0, 1 << 40, (1, K)))
    check_sums(values, np.zeros((1, K), np.int32), 3, np.full((1, K), 1 << 15, np.int32))      # one accumulator takes every add


@pytest.mark.parametrize("K", [257, 1600])
def test_sums_into_one_group_and_by_the_identity(K):
    rng = np.random.default_rng(K + 1)
    values = spread_values(rng, (3, 3, K), -60, 60)
    counts = rng.integers(1, 100, (3, K)).astype(np.int32)
    got = check_sums(values, np.full((3, K), 4, np.int32), 5, counts)
    assert not got[:, :, :4].any() and got[:, :, 4].all()
    ident = np.tile(np.arange(K, dtype=np.int32), (3, 1))
    same_values, same_counts = group_sums(dev(values), dev(ident), K, dev(counts))
    assert np.array_equal(bits(same_values), bits(values)) and np.array_equal(same_counts.cpu().numpy(), counts)
    wider = check_sums(values, ident, K + 7)
    assert not wider[:, :, K:].any() and not np.signbit(wider[:, :, K:].cpu().numpy()).any()   # empty groups: +0.0


def test_sums_that_cancel_across_120_binary_orders():
    """Every group holds pairs x, -x with |x| from 2^-60 to 2^60 and one value r that is left over: the exact sum is r, the float64 sum
    of the same values in their order is not."""
    rng = np.random.default_rng(11)
    N, Cc, groups, pairs = 2, 3, 40, 12
    K = groups * (2 * pairs + 1)
    x = spread_values(rng, (N, Cc, groups, pairs), -60, 60)
    r = spread_values(rng, (N, Cc, groups, 1), -60, -30)
    values = np.concatenate([x, r, -x], axis=3)
    perm = rng.permutation(K)
    values = values.reshape(N, Cc, K)[:, :, perm]
    mapping = np.tile((np.arange(K) // (2 * pairs + 1))[perm].astype(np.int32), (N, 1))
    model = R.group_sums(values, mapping, groups)
    assert np.array_equal(bits(model), bits(r[..., 0]))
    f64 = np.zeros((N, Cc, groups))
    for v in range(K):
        f64[:, :, mapping[0, v]] += values[:, :, v].astype(np.float64)
    assert (f64.astype(F32) != r[..., 0]).mean() > 0.5                     # the float64 sum is wrong for most groups
    got = check_sums(values, mapping, groups)
    assert np.array_equal(bits(got), bits(r[..., 0]))


def sums_inputs():
    rng = np.random.default_rng(21)
    N, Cc, K, K2 = 3, 5, 1000, 37
    return (dev(spread_values(rng, (N, Cc, K))), dev(rng.integers(-1, K2 + 1, (N, K)).astype(np.int32)), K2,
            dev(rng.integers(0, 1 << 33, (N, K))))


def test_sums_are_the_same_from_run_to_run_and_leave_their_inputs():
    values, mapping, K2, counts = sums_inputs()
    keep = [t.clone() for t in (values, mapping, counts)]
    first = group_sums(values, mapping, K2, counts)
    for _ in range(3):
        again = group_sums(values, mapping, K2, counts)
        assert np.array_equal(bits(first[0]), bits(again[0])) and torch.equal(first[1], again[1])
    assert all(torch.equal(x, y) for x, y in zip(keep, (values, mapping, counts)))
    want, want_c = R.group_sums(values.cpu().numpy(), mapping.cpu().numpy(), K2, counts.cpu().numpy())
    assert np.array_equal(bits(first[0]), bits(want)) and np.array_equal(first[1].cpu().numpy(), want_c)
    strided = values.transpose(1, 2).contiguous().transpose(1, 2)          # a view that is not contiguous
    assert not strided.is_contiguous() and np.array_equal(bits(group_sums(strided, mapping, K2)), bits(first[0]))


# ---- edge_weights ----
def weight_case(rng, N, K, Cc, E, big_counts=False, dtype=np.int32):
    """A graph dict of random node pairs (any pairs will do for the weights), sums and counts."""
    ei = rng.integers(0, K, (2, E)).astype(np.int64)
    cuts = np.sort(rng.integers(0, E + 1, N - 1))
    g = dict(edge_index=ei, boundary=np.ones(E, np.int64), contrast=None, offsets=np.concatenate([[0], cuts, [E]]).astype(np.int64))
    counts = (rng.integers(1 << 24, 1 << 30, (N, K)) | 1 if big_counts else rng.integers(1, 2000, (N, K))).astype(dtype)
    sums = (rng.random((N, Cc, K)) * 255.0 * counts[:, None].astype(np.float64)).astype(F32)
    return g, sums, counts


def check_weights(g, sums, counts, K):
    out = []
    for mode in ("mean", "ward"):
        want = R.edge_weights(g, sums, counts, mode)
        got = edge_weights(to_graph(g, K), dev(sums), dev(counts), mode)
        assert got.dtype == torch.float32 and got.device == DEV and tuple(got.shape) == want.shape
        assert np.array_equal(bits(got), bits(want)), mode
        out.append(want)
    return out


@pytest.mark.parametrize("E", [0, 1, 255, 256, 257])
def test_weights_around_a_block(E):
    rng = np.random.default_rng(E)
    for Cc in (1, 3, 17):
        for N, K in ((1, 9), (3, 300)):
            g, sums, counts = weight_case(rng, N, K, Cc, E, dtype=np.int64 if Cc == 3 else np.int32)
            mean, ward = check_weights(g, sums, counts, K)
            assert np.isfinite(mean).all() and (E < 2 or (mean > 0).any())      # (a pair may be a node and itself: 0)
    g, sums, counts = weight_case(rng, 1, 9, 2, E)                         # [C, K] sums and [K] counts with N = 1
    assert np.array_equal(bits(edge_weights(to_graph(g, 9), dev(sums[0]), dev(counts[0]), "ward")), bits(R.edge_weights(g, sums, counts, "ward")))


def test_weights_of_more_edges_than_a_launch_has_threads():
    rng = np.random.default_rng(3)
    E = 2048 * 256 + 1000
    g, sums, counts = weight_case(rng, 3, 500, 3, E)
    assert E > 2048 * 256 and 0 < g["offsets"][1] < g["offsets"][2] < E
    mean, ward = check_weights(g, sums, counts, 500)
    assert len(np.unique(mean)) > E // 4


def test_weights_of_absent_nodes_and_nodes_out_of_range():
    rng = np.random.default_rng(4)
    K = 50
    g, sums, counts = weight_case(rng, 2, K, 3, 400)
    counts[0, [3, 7]] = 0                                                  # absent
    counts[1, [5, 9]] = (-1, -(1 << 31))                                   # and counts below zero
    bad = np.array([-1, K, K + 5, 1 << 40, -(1 << 40), 65535])
    g["edge_index"][0, 10:16] = bad                                        # a outside [0, K)
    g["edge_index"][1, 20:26] = bad                                        # b outside
    g["edge_index"][:, 30] = (-1, K)                                       # both
    mean, ward = check_weights(g, sums, counts, K)
    for w in (mean, ward):
        assert np.isposinf(w[10:16]).all() and np.isposinf(w[20:26]).all() and np.isposinf(w[30])
        assert np.isposinf(w).sum() > 13 and np.isfinite(w).sum() > 300 and not np.isnan(w).any()
    a, b = g["edge_index"]
    f = R.frame_of_edges(g)
    touched = ((f == 0) & (np.isin(a, [3, 7]) | np.isin(b, [3, 7]))) | ((f == 1) & (np.isin(a, [5, 9]) | np.isin(b, [5, 9])))
    assert touched.any() and np.isposinf(mean[touched]).all()


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_weights_with_counts_above_2_to_the_24(dtype):
    """Such a count is not a float32: the conversion rounds to nearest, ties to even, as numpy's."""
    rng = np.random.default_rng(6)
    g, sums, counts = weight_case(rng, 2, 60, 3, 500, big_counts=True, dtype=dtype)
    counts[0, :4] = ((1 << 24) + 1, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6)       # ties: down to even, up to even
    if dtype == np.int64:
        counts[1, :3] = ((1 << 40) + (1 << 16), (1 << 40) + 3 * (1 << 16), (1 << 62) + 12345)
    assert (counts.astype(F32).astype(np.float64) != counts).any()
    check_weights(g, sums, counts, 60)


# ---- limit_joins ----
def check_limit(g, K, w, join, quota, dtype=torch.int64):
    want = R.limit_joins(g, w, join, quota)
    got = limit_joins(to_graph(g, K), dev(np.asarray(w, F32)), dev(np.asarray(join, bool)), torch.tensor(list(quota), dtype=dtype, device=DEV))
    assert got.dtype == torch.bool and got.device == DEV and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)
    return want


@functools.lru_cache(maxsize=None)
def limit_case():
    maps, _ = map_case("blocky", 33, 130)
    return rag_ref.graph(maps, 40, 8)


def test_limit_quotas():
    g = limit_case()
    E = g["boundary"].shape[0]
    rng = np.random.default_rng(8)
    w = (rng.random(E) * 10).astype(F32)
    join = M.best_edges(g, w)
    joined = [int(join[lo:hi].sum()) for lo, hi in M.frames_of(g)]
    assert min(joined) > 5
    for quota in ([0, 0], [1, 1], joined, [j + 1 for j in joined], [10 ** 12, -5], [3, joined[1] - 1], [joined[0], 0]):
        kept = check_limit(g, 40, w, join, quota)
        assert [int(kept[lo:hi].sum()) for lo, hi in M.frames_of(g)] == [max(min(q, j), 0) for q, j in zip(quota, joined)]
        n = merge_components(to_graph(g, 40), dev(kept))[1].tolist()       # the forest: each kept edge removes exactly one group
        assert n == [40 - max(min(q, j), 0) for q, j in zip(quota, joined)]
    check_limit(g, 40, w, join, [4, 2], torch.int32)
    check_limit(g, 40, w, np.ones(E, bool), [7, 1000])                     # any join will do, not only a round's
    single = rag_ref.graph(map_case("blocky", 33, 130)[0][1], 40, 8)      # N = 1
    ws = w[:single["boundary"].shape[0]]
    check_limit(single, 40, ws, M.best_edges(single, ws), [5])


def test_limit_ties_zeros_and_infinities():
    g = limit_case()
    E = g["boundary"].shape[0]
    rng = np.random.default_rng(9)
    ones = np.ones(E, F32)
    join = M.best_edges(g, ones)
    kept = check_limit(g, 40, ones, join, [6, 9])                          # equal weights: the lowest positions
    for (lo, hi), q in zip(M.frames_of(g), (6, 9)):
        assert np.array_equal(np.flatnonzero(kept[lo:hi]), np.flatnonzero(join[lo:hi])[:q])
    w = rng.integers(0, 3, E).astype(F32)
    check_limit(g, 40, w, M.best_edges(g, w), [11, 13])
    signed = np.where(rng.random(E) < 0.5, F32(-0.0), F32(0.0)).astype(F32)
    kept = check_limit(g, 40, signed, join, [6, 9])                        # -0.0 is +0.0: the position decides
    assert np.array_equal(kept, check_limit(g, 40, np.zeros(E, F32), join, [6, 9]))
    mixed = np.where(rng.random(E) < 0.5, F32(-0.0), F32(1e-30)).astype(F32)
    check_limit(g, 40, mixed, join, [6, 9])                                # and below any positive weight
    inf = (rng.random(E) * 10).astype(F32)
    inf[rng.random(E) < 0.5] = np.inf
    everything = np.ones(E, bool)
    kept = check_limit(g, 40, inf, everything, [E, E])                     # +inf edges are never kept
    assert np.array_equal(kept, np.isfinite(inf))
    check_limit(g, 40, inf, everything, [5, 2])
    check_limit(g, 40, np.full(E, np.inf, F32), everything, [5, 2])
    empty = dict(edge_index=np.zeros((2, 0), np.int64), boundary=np.zeros(0, np.int64), contrast=None, offsets=np.zeros(3, np.int64))
    assert tuple(check_limit(empty, 5, np.zeros(0, F32), np.zeros(0, bool), [1, 1]).shape) == (0,)


# ---- merge_hierarchical ----
@functools.lru_cache(maxsize=None)
def hierarchy_case(kind, H, W, connectivity):
    """The maps (labels of -1 and >= K present), the features of a uint8 image, and the pooled sums and counts on both sides."""
    K = 40
    maps, image = map_case(kind, H, W)
    assert (maps == -1).any() and (maps >= K).any()
    labels, img = dev(maps), dev(image)
    features = img.permute(0, 3, 1, 2).float().contiguous()                # [N, 3, H, W], integers 0 .. 255
    sums, counts = superpixel_pool(features, labels, K, reduce="sum", return_counts=True)
    g = superpixel_graph(labels, K, connectivity, img)
    d = rag_ref.graph(maps, K, connectivity, image)
    msums = np.stack([[np.bincount(m[(m >= 0) & (m < K)], weights=image[f][..., c][(m >= 0) & (m < K)], minlength=K) for c in range(3)]
                      for f, m in enumerate(maps)]).astype(F32)
    mcounts = np.stack([np.bincount(m[(m >= 0) & (m < K)], minlength=K) for m in maps]).astype(np.int32)
    assert msums.max() < 1 << 24 and np.array_equal(bits(sums), bits(msums)) and np.array_equal(counts.cpu().numpy(), mcounts)
    assert M.same_graph(to_dict(g), d)
    return K, labels, img, features, g, sums, counts, d, msums, mcounts


def check_result(res, want, K):
    assert isinstance(res, MergeResult)
    assert res.mapping.dtype == torch.int32 and res.n.dtype == torch.int32 and res.sums.dtype == torch.float32
    assert np.array_equal(res.mapping.cpu().numpy(), want["mapping"]) and np.array_equal(res.n.cpu().numpy(), want["n"])
    assert M.same_graph(to_dict(res.graph), want["graph"]) and res.graph.num_components == K
    assert np.array_equal(bits(res.sums), bits(want["sums"])) and np.array_equal(res.counts.cpu().numpy(), want["counts"])


def options(H):
    """A threshold alone, a target alone, both, Ward's weights, neither.  The threshold lets some regions of these maps join and not
    all: the larger regions of the larger map have means that lie closer."""
    t = 10.0 if H == 37 else 5.0
    return [dict(threshold=t), dict(target=9), dict(threshold=2 * t, target=15), dict(threshold=3000.0, mode="ward", max_rounds=3), dict()]


@pytest.mark.parametrize("kind", ["blocky", "noise"])
@pytest.mark.parametrize("H,W", [(37, 53), (70, 130)])
def test_hierarchy(kind, H, W):
    connectivity = 4 if kind == "blocky" else 8
    K, labels, img, features, g, sums, counts, d, msums, mcounts = hierarchy_case(kind, H, W, connectivity)
    keep = [t.clone() for t in (g.edge_index, g.boundary, g.contrast, g.offsets, sums, counts)]
    present = (mcounts > 0).sum(1)
    for kw in options(H):
        want = R.merge_hierarchical(d, msums, mcounts, **kw)
        res = merge_hierarchical(g, sums, counts, **kw)
        check_result(res, want, K)
        n = want["n"]
        if "target" in kw:
            assert (n >= np.minimum(kw["target"], present)).all()
        if kw == dict(target=9):
            assert n.tolist() == [9, 9]                                    # connected maps: the target is met exactly
        # the regions against the pixels: a re-pool of the relabelled map, and the graph of the relabelled map
        coarse = merge_labels(labels, res.mapping)
        psums, pcounts = superpixel_pool(features, coarse, K, reduce="sum", return_counts=True)
        assert torch.equal(res.counts, pcounts) and np.array_equal(bits(res.sums), bits(psums))
        assert same(res.graph, superpixel_graph(coarse, K, connectivity, img))
        # the invariant of rule 4
        s, c = group_sums(sums, res.mapping, K, counts)
        assert np.array_equal(bits(res.sums), bits(s)) and torch.equal(res.counts, c)
    assert all(torch.equal(x, y) for x, y in zip(keep, (g.edge_index, g.boundary, g.contrast, g.offsets, sums, counts)))
    n = R.merge_hierarchical(d, msums, mcounts, **options(H)[0])["n"]
    assert n.max() < present.min() and n.min() > 1                         # the threshold does merge, and not everything


@pytest.mark.parametrize("kind,H,W", [("blocky", 37, 53), ("noise", 70, 130)])
def test_hierarchy_features_do_not_depend_on_the_route(kind, H, W):
    """Features that are no integers (node sums with 24 significant bits): a region's feature is one rounding of the exact sum of its
    original nodes, whether one, two or eight rounds formed it."""
    K, labels, img, features, g, sums, counts, d, msums, mcounts = hierarchy_case(kind, H, W, 4)
    rng = np.random.default_rng(H)
    fsums = (msums.astype(np.float64) * (1.0 + rng.random(msums.shape)) / 3.0).astype(F32)
    fs = dev(fsums)
    runs = {}
    for target in (1, 6):
        for rounds in (1, 2, 8):
            want = R.merge_hierarchical(d, fsums, mcounts, target=target, max_rounds=rounds)
            res = merge_hierarchical(g, fs, counts, target=target, max_rounds=rounds)
            check_result(res, want, K)
            s, c = group_sums(fs, res.mapping, K, counts)
            assert np.array_equal(bits(res.sums), bits(s)) and torch.equal(res.counts, c)
            runs[target, rounds] = (want, res)
    assert runs[6, 8][0]["n"].tolist() == [6, 6] and runs[1, 8][0]["n"].tolist() == [1, 1]
    assert (runs[1, 1][0]["n"] > runs[1, 2][0]["n"]).all() and (runs[1, 2][0]["n"] > 1).all()        # the rounds are different routes
    assert runs[6, 8][0]["rounds"] >= 2 and runs[1, 8][0]["rounds"] > 2
    # everything in one region (target 1, enough rounds): the sum of all nodes, rounded once, whatever the rounds in between were
    whole = np.array([[pool_bits(fsums[f, c][mcounts[f] > 0]) for c in range(3)] for f in range(2)], np.uint32)
    assert np.array_equal(bits(runs[1, 8][1].sums)[:, :, 0], whole)
    # where the model says two routes end in the same regions, they have the same features
    met = 0
    for a in runs:
        for b in runs:
            if a < b and np.array_equal(runs[a][0]["mapping"], runs[b][0]["mapping"]):
                met += 1
                assert np.array_equal(bits(runs[a][1].sums), bits(runs[b][1].sums)) and torch.equal(runs[a][1].counts, runs[b][1].counts)
    # two rounds of one are the regions of a run of two rounds: by that route the node sums are rounded twice, here once
    first = merge_hierarchical(g, fs, counts, target=1, max_rounds=1)
    second = merge_hierarchical(first.graph, first.sums, first.counts, target=1, max_rounds=1)
    if np.array_equal(torch.gather(second.mapping, 1, first.mapping.clamp_min(0).long()).cpu().numpy()[mcounts > 0], runs[1, 2][0]["mapping"][mcounts > 0]):
        met += 1
        assert torch.equal(second.counts, runs[1, 2][1].counts)
        assert np.array_equal(bits(group_sums(fs, runs[1, 2][1].mapping, K)), bits(runs[1, 2][1].sums))
    assert met >= 1


def pool_bits(values):
    import pool_ref
    return pool_ref.exact_sum_bits(np.ascontiguousarray(values, F32).view(np.uint32).tolist())


def test_hierarchy_with_a_target_above_the_node_count_joins_nothing():
    K, labels, img, features, g, sums, counts, d, msums, mcounts = hierarchy_case("blocky", 37, 53, 4)
    present = mcounts > 0
    for target in (int(present.sum(1).max()), K + 1, 10 ** 6):
        res = merge_hierarchical(g, sums, counts, target=target)
        check_result(res, R.merge_hierarchical(d, msums, mcounts, target=target), K)
        assert res.n.tolist() == present.sum(1).tolist()
        rank = np.where(present, np.cumsum(present, axis=1) - 1, -1)       # every node its own region, numbered in order
        assert np.array_equal(res.mapping.cpu().numpy(), rank)
        assert res.graph.edge_index.shape[1] == to_dict(g)["boundary"].shape[0] - absent_edges(d, present)


def absent_edges(d, present):
    a, b = d["edge_index"]
    f = R.frame_of_edges(d)
    return int((~present[f, a] | ~present[f, b]).sum())


def test_hierarchy_of_one_frame_and_of_a_graph_without_edges():
    K, labels, img, features, g, sums, counts, d, msums, mcounts = hierarchy_case("noise", 37, 53, 8)
    one = superpixel_graph(labels[1], K, 8, img[1])
    want = R.merge_hierarchical(to_dict(one), msums[1:], mcounts[1:], threshold=16.0, target=5)
    check_result(merge_hierarchical(one, sums[1], counts[1], threshold=16.0, target=5), want, K)      # [C, K] and [K]
    check_result(merge_hierarchical(one, sums[1:], counts[1:].long(), threshold=16.0, target=5), dict(want, counts=want["counts"].astype(np.int64)), K)
    empty = dict(edge_index=np.zeros((2, 0), np.int64), boundary=np.zeros(0, np.int64), contrast=None, offsets=np.zeros(3, np.int64))
    res = merge_hierarchical(to_graph(empty, K), sums, counts, target=3)
    check_result(res, R.merge_hierarchical(empty, msums, mcounts, target=3), K)
    assert res.n.tolist() == (mcounts > 0).sum(1).tolist() and res.graph.edge_index.shape[1] == 0


# ---- streams and synchronisation ----
def single_calls(g, sums, counts, mapping, quota):
    w = edge_weights(g, sums, counts, "ward")
    join = best_neighbour_edges(g, w)
    kept = limit_joins(g, w, join, quota)
    s, c = group_sums(sums, mapping, 40, counts)
    return w, kept, s, c


def call_inputs():
    K, labels, img, features, g, sums, counts, d, msums, mcounts = hierarchy_case("blocky", 70, 130, 4)
    mapping = dev(np.random.default_rng(2).integers(-1, 12, (2, K)).astype(np.int32))
    return g, sums, counts, mapping, torch.tensor([3, 5], dtype=torch.int32, device=DEV)


def test_side_stream():
    g, sums, counts, mapping, quota = call_inputs()
    want = single_calls(g, sums, counts, mapping, quota)
    whole = merge_hierarchical(g, sums, counts, target=7)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        sums2 = sums.clone()                                               # produced on the side stream, consumed there
        got = single_calls(g, sums2, counts, mapping, quota)
        res = merge_hierarchical(g, sums2, counts, target=7)
        s.synchronize()                                                    # this stream only
        assert all(np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8)) for x, y in zip(want, got))
        assert torch.equal(res.mapping, whole.mapping) and np.array_equal(bits(res.sums), bits(whole.sums)) and same(res.graph, whole.graph)


def test_no_host_synchronisation():
    g, sums, counts, mapping, quota = call_inputs()
    want = single_calls(g, sums, counts, mapping, quota)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    got = None
    try:
        try:
            torch.ones(1, device=DEV).item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            got = single_calls(g, sums, counts, mapping, quota)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if got is None:                                                        # a torch build that does not raise on .item() under "error"
        got = single_calls(g, sums, counts, mapping, quota)
    assert all(np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8)) for x, y in zip(want, got))
