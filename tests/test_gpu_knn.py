"""knn_graph on the MI355X (fast_slic_amd/knn.py, csrc/knn.hip) against the model written from the rule (tests/knn_ref.py): indices and
distances compared byte for byte, at node counts around a wavefront, a block and a candidate tile, every k and D at which the kernel
takes another form (256 and 128 threads, the two register forms and the global one, 16 and 64 rows a block), ties on purpose (an integer
grid, equal points, duplicates across tile and slice boundaries), masks, NaN and infinities, `other`, the loop, strided views, the same
bits from run to run and in both directions, a side stream, and the lists fed to graph_aggregate and graph_attention against their
models."""
import numpy as np
import pytest
import torch

import aggregate_ref as A
import attention_ref as AT
import knn_ref as M
from fast_slic_amd.attention import graph_attention
from fast_slic_amd.knn import knn_graph
from fast_slic_amd.propagate import NeighbourLists, graph_aggregate

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def normal(seed, N, D, K):
    return np.random.default_rng(seed).standard_normal((N, D, K)).astype(F32)


def check(points, k, other=None, valid=None, loop=False):
    """One call against the model, byte for byte, and the shape of what comes back -> (indices, dist) as numpy arrays."""
    N, D, K = points.shape
    pt = dev(points)
    ot = None if other is None else pt if other is points else dev(other)
    nl, dist = knn_graph(pt, k, other=ot, valid=None if valid is None else dev(valid), loop=loop)
    assert isinstance(nl, NeighbourLists) and nl.edge is None and (nl.num_frames, nl.num_components) == (N, K)
    assert nl.indices.dtype == torch.int32 and dist.dtype == torch.float32 and nl.indices.shape == dist.shape == (N * K * k,)
    assert nl.indices.device == dist.device == nl.offsets.device == nl.rows.device == DEV and not dist.requires_grad
    assert nl.offsets.dtype == torch.int64 and torch.equal(nl.offsets, torch.arange(N * K + 1, device=DEV) * k)
    assert nl.rows.dtype == torch.int32 and torch.equal(nl.rows, torch.arange(N * K, dtype=torch.int32, device=DEV).repeat_interleave(k))
    want_i, want_d = M.knn(points, k, other=other, valid=valid, loop=loop)
    got_i, got_d = host(nl.indices), host(dist)
    assert got_i.tobytes() == want_i.tobytes(), "indices"
    assert got_d.tobytes() == want_d.tobytes(), "distances"
    return got_i, got_d


# ---- node counts, k, D and the forms they select ----
@pytest.mark.parametrize("N,D,K,k", [
    (1, 3, 1, 4),                                                          # K = 1: every row is padding
    (1, 2, 2, 1),
    (2, 3, 63, 5), (2, 3, 64, 5), (2, 3, 65, 5),                           # around a wavefront
    (1, 4, 255, 7), (1, 4, 257, 7),                                        # around a block
    (2, 5, 1601, 16),                                                      # several tiles (816 candidates) and slices, a ragged last one
    (1, 3, 40, 1), (1, 3, 40, 16), (1, 3, 40, 17), (1, 3, 40, 32),         # k = 1, the last of 256 threads, the first of 128, the largest
    (1, 3, 33, 32), (2, 3, 9, 8),                                          # k = K - 1, in both block sizes
    (1, 3, 20, 32), (2, 3, 9, 16),                                         # k > K - 1
    (1, 1, 100, 4), (1, 8, 100, 4), (1, 9, 100, 4),                        # D = 1; the last D of the narrow register form and the first of the wide
    (2, 33, 300, 6), (2, 33, 300, 20),                                     # D = 33: tiles of 112 candidates
    (1, 64, 200, 6), (1, 65, 70, 6), (2, 130, 70, 20),                     # the last D of the register form, the first and one more of the global form
])
def test_shapes_in_blocks_of_16_rows(N, D, K, k):
    check(normal(N * 1000 + D * 10 + k, N, D, K), k)


@pytest.mark.parametrize("N,D,K,k", [(128, 3, 65, 32), (90, 64, 130, 8), (128, 130, 70, 4), (16, 5, 1025, 16)])
def test_shapes_in_blocks_of_64_rows(N, D, K, k):
    """N * ceil(K / 64) >= 256: a wave is one slice.  128 and 256 threads, three tiles of 64 candidates, the global form, two tiles
    of 816 with a group of one row; a mask and duplicates of node 0 in every frame."""
    x = normal(K + k, N, D, K)
    x[:, :, [K // 2, K - 1]] = x[:, :, [0]]
    valid = np.random.default_rng(k).random((N, K)) < 0.9
    check(x, k)
    check(x, k, valid=valid, loop=True)


def test_three_frames_one_of_them_without_a_valid_node():
    x = normal(3, 3, 4, 90)
    x[1] *= 100
    valid = np.ones((3, 90), bool)
    valid[2] = False
    valid[0, ::3] = False
    ind, d = check(x, 6, valid=valid)
    assert (ind.reshape(3, 90, 6)[2] == -1).all() and np.isinf(d.reshape(3, 90, 6)[2]).all()


# ---- ties on purpose: where a merge that is not by key goes wrong ----
@pytest.mark.parametrize("k", [8, 32])
def test_integer_grid_with_many_equal_distances(k):
    yy, xx = np.mgrid[0:20, 0:20]
    x = np.stack([yy.ravel(), xx.ravel()]).astype(F32)[None]               # [1, 2, 400]
    ind, d = check(x, k)
    d = d.reshape(400, k)
    assert (d[:, :2] == 1).all() and (d[:, 1:] == d[:, :-1]).mean() > 0.5  # most neighbours tie with the one before
    check(np.concatenate([x, x[:, ::-1]]), k, loop=True)


@pytest.mark.parametrize("k", [16, 17])
def test_equal_points_give_the_smallest_indices(k):
    ind, d = check(np.full((2, 3, 300), F32(1.25)), k)
    ind = ind.reshape(2, 300, k)
    assert not d.any() and not np.signbit(d).any()
    assert ind[0, 0].tolist() == list(range(1, k + 1)) and ind[1, 299].tolist() == list(range(k)) and ind[0, 5, :6].tolist() == [0, 1, 2, 3, 4, 6]


@pytest.mark.parametrize("D,k", [(5, 6), (64, 6), (33, 20), (70, 6)])
def test_duplicates_across_tile_and_slice_boundaries(D, k):
    """Nodes 63 / 64 and 255 / 256 are copies of node 0 (D = 64: tiles of 64 candidates; D = 33: of 112), and 111 / 112 of node 1."""
    x = normal(D, 2, D, 300)
    x[:, :, [63, 64, 255, 256]] = x[:, :, [0]]
    x[:, :, [111, 112]] = x[:, :, [1]]
    ind, d = check(x, k)
    ind, d = ind.reshape(2, 300, k), d.reshape(2, 300, k)
    assert ind[0, 0, :4].tolist() == [63, 64, 255, 256] and ind[1, 64, :4].tolist() == [0, 63, 255, 256] and not d[:, 0, :4].any()
    assert ind[0, 112, :2].tolist() == [1, 111]
    check(x, k, loop=True)


# ---- masks and special values ----
def test_fewer_valid_nodes_than_k():
    x = normal(11, 2, 3, 100)
    valid = np.zeros((2, 100), bool)
    valid[0, [3, 40, 64, 65, 99]] = True
    valid[1, 7] = True
    ind, d = check(x, 8, valid=valid)
    ind = ind.reshape(2, 100, 8)
    assert sorted(ind[0, 3, :4].tolist()) == [40, 64, 65, 99] and (ind[0, 3, 4:] == -1).all() and (ind[1] == -1).all() and (ind[0, 0] == -1).all()
    check(x, 8, valid=valid, loop=True)


def test_nan_and_infinities():
    x = normal(12, 2, 4, 130)
    x[0, 1, 5] = np.nan                                                    # a NaN in one channel: node 5 of frame 0 is a whole NaN node to everyone
    x[0, :, 70] = np.nan                                                   # a whole NaN node
    x[0, 2, 9] = np.inf                                                    # +inf in one channel: an ordinary, largest distance
    x[0, 2, 10] = -np.inf
    x[1, 0, 64] = np.inf
    x[1, 0, 65] = np.inf                                                   # inf - inf between the two: NaN, no candidate of each other
    for k in (3, 32):
        ind, d = check(x, k)
        ind, d = ind.reshape(2, 130, k), d.reshape(2, 130, k)
        assert (ind[0, [5, 70]] == -1).all() and np.isinf(d[0, [5, 70]]).all()
        assert not np.isin(ind[0], [5, 70]).any() and not np.isin(ind[1, 64], [65]).any()
        assert np.isinf(d[1, 64]).all() and (ind[1, 64] >= 0).all()
    ind, d = check(x[:, :, :20], 19)                                       # k = K - 1: the infinite distances come last, NaN pairs are padding
    assert np.isinf(d.reshape(2, 20, 19)[0, 0, -2:]).all()
    check(x, 5, loop=True)
    check(x, 5, other=x[::-1].copy())


# ---- other, the loop, views ----
def test_other_and_the_loop():
    x, y = normal(20, 2, 5, 200), normal(21, 2, 5, 200)
    y[:, :, 150:] = x[:, :, :50]
    valid = np.random.default_rng(1).random((2, 200)) < 0.7
    check(x, 8, other=y)
    check(x, 20, other=y, valid=valid)
    ind, d = check(x, 4, other=x)                                          # other is points: the node itself first, at +0
    assert (ind.reshape(400, 4)[:, 0] == np.tile(np.arange(200), 2)).all() and not d.reshape(400, 4)[:, 0].any()
    ind2, d2 = check(x, 4, loop=True)
    assert ind2.tobytes() == ind.tobytes() and d2.tobytes() == d.tobytes()
    check(x, 4, other=x.copy())                                            # and so does an equal tensor


def test_strided_views_and_the_unbatched_form():
    base = dev(normal(30, 3, 140, 12))                                     # [N, K, D]
    view = base.transpose(1, 2)[:, ::2, 3:]                                # [3, 6, 137], nothing contiguous
    assert not view.is_contiguous()
    valid = dev(np.random.default_rng(2).random((3, 200)) < 0.8)[:, 5:142]
    nl, dist = knn_graph(view, 7, valid=valid, other=view.flip(0))
    want_i, want_d = M.knn(host(view), 7, other=host(view.flip(0)), valid=host(valid))
    assert host(nl.indices).tobytes() == want_i.tobytes() and host(dist).tobytes() == want_d.tobytes()
    one = view[1]
    nl, dist = knn_graph(one, 7, valid=valid[1])
    want_i, want_d = M.knn(host(one)[None], 7, valid=host(valid[1])[None])
    assert (nl.num_frames, nl.num_components) == (1, 137) and host(nl.indices).tobytes() == want_i.tobytes() and host(dist).tobytes() == want_d.tobytes()


# ---- reproducible, symmetric, on any stream ----
def test_the_same_bits_from_run_to_run_and_in_both_directions():
    x = dev(normal(40, 2, 5, 1601))
    x[:, :, 800:1000] = x[:, :, :200]
    (a, da), (b, db) = knn_graph(x, 16), knn_graph(x, 16)
    assert torch.equal(a.indices, b.indices) and torch.equal(da.view(torch.int32), db.view(torch.int32))
    # d(i, j) is d(j, i) bit for bit wherever both entries appear
    K, k = 1601, 16
    ind, d = host(a.indices).reshape(2, K, k).astype(np.int64), host(da).view(np.uint32).reshape(2, K, k)
    both = 0
    for f in range(2):
        table = {}
        for i, o in zip(*np.nonzero(ind[f] >= 0)):
            table[(i, ind[f, i, o])] = d[f, i, o]
        pairs = [(key, v) for key, v in table.items() if (key[1], key[0]) in table]
        assert all(table[(j, i)] == v for (i, j), v in pairs)
        both += len(pairs)
    assert both > 2 * K


def test_side_stream_and_no_host_synchronisation():
    x, y = dev(normal(50, 2, 6, 300)), dev(normal(51, 2, 6, 300))
    valid = dev(np.random.default_rng(3).random((2, 300)) < 0.8)

    def calls():
        out = []
        for kw in (dict(), dict(other=y, valid=valid), dict(loop=True, valid=valid)):
            nl, dist = knn_graph(x, 9, **kw)
            out += [nl.indices, dist, nl.offsets, nl.rows]
        return out

    want = calls()
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
            got = calls()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    stream = torch.cuda.Stream(DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        side = calls()
        stream.synchronize()                                               # this stream only
    for other in (got, side):
        assert other is None or all(host(a).tobytes() == host(b).tobytes() for a, b in zip(want, other))


# ---- the lists on the chain ----
def chain_case():
    N, D, K, k = 2, 6, 70, 5
    pts = normal(60, N, D, K)
    valid = np.random.default_rng(4).random((N, K)) < 0.85
    valid[1, 3:] = False                                                   # frame 1: three valid nodes, every row padded
    nl, dist = knn_graph(dev(pts), k, valid=dev(valid))
    offsets, indices = host(nl.offsets), host(nl.indices)
    assert (indices == -1).any() and (indices >= 0).any()
    return N, K, nl, dist, offsets, indices


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_graph_aggregate_on_the_padded_lists(reduce):
    N, K, nl, dist, offsets, indices = chain_case()
    rng = np.random.default_rng(5)
    x, g = (rng.standard_normal((N, 9, K)).astype(F32) for _ in range(2))
    wt = torch.exp(-dist).requires_grad_() if reduce == "sum" else None     # a Gaussian weight: +0 on the padding
    w = host(wt) if wt is not None else None
    xt = dev(x).requires_grad_()
    y = graph_aggregate(xt, nl, weight=wt, reduce=reduce)
    y.backward(dev(g))
    want, argmax, degree = A.forward(x, offsets, indices, w, reduce)
    assert host(y).tobytes() == want.tobytes()
    assert host(xt.grad).tobytes() == A.backward_values(g, offsets, indices, w, reduce, argmax, degree).tobytes()
    if wt is not None:
        assert host(wt.grad).tobytes() == A.backward_weight(x, g, offsets, indices).tobytes()


def test_graph_attention_on_the_padded_lists():
    N, K, nl, dist, offsets, indices = chain_case()
    rng = np.random.default_rng(6)
    q, kk, v, gy = (rng.standard_normal((N, 8, K)).astype(F32) for _ in range(4))
    qt, kt, vt = (dev(t).requires_grad_() for t in (q, kk, v))
    y = graph_attention(qt, kt, vt, nl, heads=2)
    y.backward(dev(gy))
    want_y, _, grads = AT.attention(q, kk, v, AT.Entries(offsets, indices, N, K), 2, None, gy=gy)
    assert host(y).tobytes() == want_y.tobytes()
    assert all(host(t.grad).tobytes() == want.tobytes() for t, want in zip((qt, kt, vt), grads))
