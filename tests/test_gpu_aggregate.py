"""Aggregation over neighbour lists on the MI355X (fast_slic_amd/propagate.py, csrc/aggregate.hip) against the model written from
the rules (tests/aggregate_ref.py), with exact equality throughout: forward, grad_values and grad_weight of the sum, forward and
grad_values of the mean, forward, argmax and grad_values of the max with deliberate ties, on paths, stars whose hub is longer than a
wavefront, than a block and than the kernel's LDS window, random graphs, isolated nodes, frames without an edge, the graph of a label
map, node counts around a block and channel counts around the 8 of a wave and the 32 of an item; non-contiguous and unbatched values,
a raw pair with invalid entries, once round each kernel's loop, a side stream without host synchronisation, the same bits from run to
run, entry_values as weights end to end, and the weighted sum below 32 channels against head_aggregate's other item shape."""
import numpy as np
import pytest
import torch

import aggregate_ref as A
import connect_ref
from fast_slic_amd.attention import head_aggregate
from fast_slic_amd.propagate import graph_aggregate, neighbour_lists
from fast_slic_amd.rag import superpixel_graph
from test_aggregate_cpu import make_graph, numpy_lists, path, random_pairs, star

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(got, want):
    return tuple(got.shape) == tuple(np.shape(want)) and np.array_equal(bits(got), bits(want))


def tied_values(rng, shape):
    """Few distinct values, so that most rows hold their maximum more than once; channel 0 is constant."""
    x = rng.integers(-2, 3, shape).astype(F32)
    x[:, 0] = F32(1.5)
    return x


def run(x, lists, weight, reduce, g):
    """One forward and backward on the GPU -> (y, argmax, grad_values, grad_weight)."""
    xt = dev(x).requires_grad_()
    wt = dev(weight).requires_grad_() if weight is not None else None
    if reduce == "max":
        y, arg = graph_aggregate(xt, lists, wt, reduce, return_argmax=True)
        assert arg.dtype == torch.int32 and not arg.requires_grad
    else:
        y, arg = graph_aggregate(xt, lists, wt, reduce), None
    assert y.dtype == torch.float32 and y.device == DEV and y.shape == xt.shape and y.requires_grad
    y.backward(dev(g))
    with torch.no_grad():                                                  # outside autograd: the same launch, the same bits
        assert torch.equal(graph_aggregate(xt, lists, wt, reduce).view(torch.int32), y.detach().view(torch.int32))
    return y, arg, xt.grad, wt.grad if wt is not None else None


def check(lists, offsets, indices, N, K, Cc, seed=0, reduces=("sum", "weighted", "mean", "max")):
    """Every reduction on `lists` (NeighbourLists, a graph or a pair on the GPU; offsets and indices the same lists in numpy)."""
    rng = np.random.default_rng(seed)
    x, g = rng.standard_normal((N, Cc, K)).astype(F32), rng.standard_normal((N, Cc, K)).astype(F32)
    w = rng.standard_normal(len(indices)).astype(F32)
    for reduce in reduces:
        weight, red = (w, "sum") if reduce == "weighted" else (None, reduce)
        xin = tied_values(rng, (N, Cc, K)) if red == "max" else x
        want, want_arg, deg = A.forward(xin, offsets, indices, weight, red)
        y, arg, gx, gw = run(xin, lists, weight, red, g)
        assert same(y, want), reduce
        if red == "max":
            assert np.array_equal(arg.cpu().numpy(), want_arg)
        assert same(gx, A.backward_values(g, offsets, indices, weight, red, want_arg, deg)), reduce
        if weight is not None:
            assert same(gw, A.backward_weight(xin, g, offsets, indices))


def check_graph(frames, K, Cc, seed=0, **kw):
    g = make_graph(frames, K, DEV, seed)
    nl = neighbour_lists(g)
    check(nl, *numpy_lists(nl), len(frames), K, Cc, seed, **kw)
    return g, nl


# ---- graphs ----
@pytest.mark.parametrize("K", [1, 2, 255, 256, 257])
def test_paths_and_random_graphs_around_a_block(K):
    rng = np.random.default_rng(K)
    check_graph([path(K)], K, 3)
    # three frames with different edge counts, one of them without an edge; nodes 0 and K - 1 and a few more are isolated
    isolated = {0, K - 1} | set(rng.integers(0, K, 5).tolist())
    check_graph([random_pairs(rng, K, 6, isolated), [], random_pairs(rng, K, 2)], K, 5, seed=K)
    check_graph([random_pairs(rng, K, 9)], K, 1, seed=K + 1)


@pytest.mark.parametrize("K,degree", [(400, 300), (1100, 1025)])
def test_star_hubs_longer_than_a_wavefront_a_block_and_the_window(K, degree):
    """The hub's row (and, transposed, its target) is walked in full and in order, and the rows behind it in its tile start beyond the
    LDS window."""
    rng = np.random.default_rng(degree)
    g, nl = check_graph([star(K, degree)], K, 3)
    check_graph([star(K, degree, hub=5) + random_pairs(rng, K, 4), path(K)], K, 2, seed=1)
    # the weight's gradient where the hub's entries share one row: every thread of many wavefronts reads the same cells of grad_out
    offsets, indices = numpy_lists(nl)
    hub = int(np.argmax(np.diff(offsets)))
    assert offsets[hub + 1] - offsets[hub] == degree and (nl.rows[offsets[hub]:offsets[hub + 1]] == hub).all()
    x, gout = rng.standard_normal((1, 3, K)).astype(F32), rng.standard_normal((1, 3, K)).astype(F32)
    w = rng.standard_normal(len(indices)).astype(F32)
    gw = run(x, nl, w, "sum", gout)[3]
    want = A.backward_weight(x, gout, offsets, indices)
    assert same(gw, want) and want[offsets[hub]:offsets[hub + 1]].all()


def test_no_edges():
    for N, K, Cc in ((1, 1, 1), (2, 70, 3)):
        g, nl = check_graph([[]] * N, K, Cc)
        x = dev(np.full((N, Cc, K), -1.0, F32))
        for reduce in ("sum", "mean", "max"):
            y = graph_aggregate(x, g, reduce=reduce)                       # a graph directly: the lists are built by the call
            assert not y.any() and not np.signbit(y.cpu().numpy()).any()   # an empty row is +0.0
        assert (graph_aggregate(x, nl, reduce="max", return_argmax=True)[1] == -1).all()


@pytest.mark.parametrize("Cc", [1, 3, 64, 65])
def test_channels_around_an_item(Cc):
    rng = np.random.default_rng(Cc)
    check_graph([random_pairs(rng, 257, 6), random_pairs(rng, 257, 3), path(257)], 257, Cc, seed=Cc)


@pytest.mark.parametrize("Cc", [1, 3])
def test_weighted_sum_is_head_aggregate_at_one_head(Cc):
    """Below 32 channels the weighted sum runs the apply kernel's item of 32 channels of one head and head_aggregate its packed item:
    both are the model's bytes, and so each other's, forward and for both gradients."""
    rng = np.random.default_rng(Cc)
    nl = neighbour_lists(make_graph([random_pairs(rng, 257, 6), random_pairs(rng, 257, 3), path(257)], 257, DEV, Cc))
    offsets, indices = numpy_lists(nl)
    x, gout = rng.standard_normal((3, Cc, 257)).astype(F32), rng.standard_normal((3, Cc, 257)).astype(F32)
    w = rng.standard_normal(len(indices)).astype(F32)
    y, _, gx, gw = run(x, nl, w, "sum", gout)
    assert same(y, A.forward(x, offsets, indices, w)[0]) and same(gx, A.backward_values(gout, offsets, indices, w))
    assert same(gw, A.backward_weight(x, gout, offsets, indices))
    xt, wt = dev(x).requires_grad_(), dev(w).requires_grad_()
    yh = head_aggregate(xt, nl, wt)                                        # [nnz]: one head
    yh.backward(dev(gout))
    for a, b in ((y, yh), (gx, xt.grad), (gw, wt.grad)):
        assert a.shape == b.shape and torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


@pytest.mark.parametrize("connectivity", [4, 8])
def test_graph_of_a_label_map(connectivity):
    K = 60
    maps = np.stack([connect_ref.blocky(37, 53, K, seed=s) for s in (1, 2)])
    g = superpixel_graph(dev(maps), K, connectivity)
    nl = neighbour_lists(g)
    offsets, indices = g.to_batch_csr()
    assert torch.equal(nl.offsets, offsets) and torch.equal(nl.indices, indices) and torch.equal(nl.rows.long(), torch.repeat_interleave(nl.degree().flatten().long()))
    check(g, *numpy_lists(nl), 2, K, 3, seed=connectivity)


# ---- tensor layouts ----
def test_non_contiguous_and_unbatched_values():
    rng = np.random.default_rng(3)
    K, Cc = 130, 5
    g = make_graph([random_pairs(rng, K, 6)], K, DEV)
    nl = neighbour_lists(g)
    offsets, indices = numpy_lists(nl)
    x, gout = rng.standard_normal((1, Cc, K)).astype(F32), rng.standard_normal((1, Cc, K)).astype(F32)
    w = rng.standard_normal(len(indices)).astype(F32)
    want, want_gx = A.forward(x, offsets, indices, w)[0], A.backward_values(gout, offsets, indices, w)
    leaf = dev(x.transpose(0, 2, 1)).requires_grad_()                      # [1, K, C] in memory
    xt = leaf.transpose(1, 2)
    assert not xt.is_contiguous()
    y = graph_aggregate(xt, nl, dev(w))
    y.backward(dev(gout.transpose(0, 2, 1)).transpose(1, 2))               # a non-contiguous gradient as well
    assert same(y, want) and same(leaf.grad.transpose(1, 2), want_gx)
    one = dev(x[0]).requires_grad_()                                       # [C, K]
    y = graph_aggregate(one, nl, dev(w))
    y.backward(dev(gout[0]))
    assert tuple(y.shape) == (Cc, K) and same(y, want[0]) and same(one.grad, want_gx[0])
    ym, arg = graph_aggregate(one.detach(), g, reduce="max", return_argmax=True)
    assert tuple(arg.shape) == (Cc, K) and same(ym, A.forward(x, offsets, indices, reduce="max")[0][0])


def test_raw_pair_with_invalid_entries():
    """Entries -1 and K are ignored everywhere, and so are their weight gradients."""
    rng = np.random.default_rng(4)
    N, K, Cc = 2, 257, 4
    offsets, indices = numpy_lists(neighbour_lists(make_graph([random_pairs(rng, K, 7), random_pairs(rng, K, 5)], K)))
    indices = indices.copy()
    bad = rng.random(len(indices)) < 0.2
    indices[bad] = rng.choice([-1, K], bad.sum()).astype(np.int32)
    indices[:3], indices[-1] = (-1, K, -1), K
    bad = (indices < 0) | (indices >= K)
    pair = (dev(offsets), dev(indices))
    check(pair, offsets, indices, N, K, Cc)
    check(neighbour_lists(pair, num_frames=N, num_components=K), offsets, indices, N, K, Cc, seed=1)
    x, g, w = (rng.standard_normal(s).astype(F32) for s in ((N, Cc, K), (N, Cc, K), len(indices)))
    gw = run(x, pair, w, "sum", g)[3].cpu().numpy()
    assert bad.sum() > 50 and not gw[bad].any() and not np.signbit(gw[bad]).any() and gw[~bad].all()


# ---- once round each kernel's loop ----
def test_more_items_than_blocks():
    """13 tiles of 64 rows x 632 groups of 32 channels = 8216 items for the 8192 blocks of a launch."""
    rng = np.random.default_rng(5)
    check_graph([random_pairs(rng, 257, 4), [], path(257)], 257, 632 * 32 - 3, reduces=("weighted", "max"))


def test_more_entries_than_threads():
    """The weights' backward has 2048 blocks of 256 threads: 524288 entries a round."""
    rng = np.random.default_rng(6)
    K = 4000
    nl = neighbour_lists(make_graph([random_pairs(rng, K, 140)], K, DEV))
    offsets, indices = numpy_lists(nl)
    assert len(indices) > 2048 * 256
    x, g = rng.standard_normal((1, 2, K)).astype(F32), rng.standard_normal((1, 2, K)).astype(F32)
    w = dev(rng.standard_normal(len(indices)).astype(F32)).requires_grad_()
    graph_aggregate(dev(x), nl, w).backward(dev(g))
    assert same(w.grad, A.backward_weight(x, g, offsets, indices))


# ---- reproducibility, and the chain from the graph's edge features ----
def test_the_same_bits_from_run_to_run():
    rng = np.random.default_rng(7)
    N, K, Cc = 3, 1600, 32
    g = make_graph([random_pairs(rng, K, 6) + star(K, 700) for _ in range(N)], K, DEV)
    nl = neighbour_lists(g)
    x, gout = rng.standard_normal((N, Cc, K)).astype(F32), rng.standard_normal((N, Cc, K)).astype(F32)
    w = rng.standard_normal(nl.indices.shape[0]).astype(F32)
    for reduce, weight in (("sum", w), ("mean", None), ("max", None)):
        first, second = run(x, nl, weight, reduce, gout), run(x, nl, weight, reduce, gout)
        for a, b in zip(first, second):
            assert (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_side_stream_and_no_host_synchronisation():
    """neighbour_lists, graph_aggregate of a graph, of lists and of a raw pair, and both backwards, on a stream of the caller's and
    with torch refusing every host synchronisation: the bits of the plain call."""
    rng = np.random.default_rng(9)
    N, K, Cc = 2, 300, 5
    g = make_graph([random_pairs(rng, K, 6), random_pairs(rng, K, 4)], K, DEV)
    x, gout = dev(rng.standard_normal((N, Cc, K)).astype(F32)), dev(rng.standard_normal((N, Cc, K)).astype(F32))
    w = dev(rng.standard_normal(2 * g.edge_index.shape[1]).astype(F32))

    def calls():
        nl = neighbour_lists(g)
        xt, wt = x.clone().requires_grad_(), w.clone().requires_grad_()
        y = graph_aggregate(xt, nl, wt)
        y.backward(gout)
        xm = x.clone().requires_grad_()
        ym, arg = graph_aggregate(xm, (nl.offsets, nl.indices), reduce="max", return_argmax=True)
        ym.backward(gout)
        return y.detach(), xt.grad, wt.grad, graph_aggregate(x, g, reduce="mean"), ym.detach(), arg, xm.grad

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
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        side = calls()
        s.synchronize()                                                    # this stream only
    for other in (got, side):
        assert other is None or all(np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8)) for a, b in zip(want, other))


def test_entry_values_as_weights_end_to_end():
    K, Cc = 60, 6
    rng = np.random.default_rng(8)
    maps = np.stack([connect_ref.blocky(37, 53, K, seed=s) for s in (3, 4, 5)])
    graph = superpixel_graph(dev(maps), K, 8)
    E = graph.edge_index.shape[1]
    nl = neighbour_lists(graph)
    offsets, indices = numpy_lists(nl)
    x, gout = rng.standard_normal((3, Cc, K)).astype(F32), rng.standard_normal((3, Cc, K)).astype(F32)
    b = graph.boundary.float().requires_grad_()
    xt = dev(x).requires_grad_()
    w = nl.entry_values(b)
    y = graph_aggregate(xt, nl, w)
    y.backward(dev(gout))
    wn = w.detach().cpu().numpy()
    assert np.array_equal(wn, graph.boundary.cpu().numpy().astype(F32)[nl.edge.cpu().numpy()])
    assert same(y, A.forward(x, offsets, indices, wn)[0]) and same(xt.grad, A.backward_values(gout, offsets, indices, wn))
    gw = A.backward_weight(x, gout, offsets, indices)
    want = np.zeros(E, F32)
    np.add.at(want, nl.edge.cpu().numpy(), gw)                             # two terms an edge: their float sum has no order
    assert same(b.grad, want) and b.grad.abs().sum() > 0
