"""Attention over neighbour lists on the MI355X (fast_slic_amd/attention.py, csrc/attend.hip) against the model written from the rules
(tests/attention_ref.py), with exact equality throughout: neighbour_dot, neighbour_softmax and head_aggregate, each forward and every
gradient, on paths, random graphs with isolated nodes and a frame without an edge at node counts around a wavefront, head widths around
the eight channels of a wave and the 32 of a block, stars whose hub is longer than a wavefront and than the LDS window, the softmax's
edges (ties, -inf, subnormal exponentials, single entries, the 1-D form), a raw pair with invalid entries, non-contiguous and unbatched
tensors, once round each kernel's loop, one head against graph_aggregate, graph_attention on the graph of a label map against the
composed model and the float64 dense attention, the same bits from run to run, a side stream without host synchronisation."""
import numpy as np
import pytest
import torch

import attention_ref as M
import connect_ref
from fast_slic_amd.attention import graph_attention, head_aggregate, neighbour_dot, neighbour_softmax
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


def check(nl, ent, Hd, D, seed=0, scores=None, steps=("dot", "softmax", "sum")):
    """The three steps on `nl` (NeighbourLists on the GPU; ent the same lists for the model), forward and every gradient."""
    rng = np.random.default_rng(seed)
    N, K, Cc = ent.N, ent.K, Hd * D
    a, b, g = (rng.standard_normal((N, Cc, K)).astype(F32) for _ in range(3))
    gs, w = (rng.standard_normal((Hd, ent.nnz)).astype(F32) for _ in range(2))
    s = rng.uniform(-8, 8, (Hd, ent.nnz)).astype(F32) if scores is None else scores
    if "dot" in steps:
        at, bt = dev(a).requires_grad_(), dev(b).requires_grad_()
        st = neighbour_dot(at, bt, nl, Hd)
        assert st.dtype == torch.float32 and st.device == DEV and st.requires_grad
        st.backward(dev(gs))
        assert same(st, M.dot(a, b, ent, Hd)), "dot"
        assert same(at.grad, M.apply(b, gs, ent)) and same(bt.grad, M.apply_transposed(a, gs, ent)), "dot gradients"
        with torch.no_grad():                                              # outside autograd: the same launch, the same bits
            assert torch.equal(neighbour_dot(at, bt, nl, Hd).view(torch.int32), st.detach().view(torch.int32))
    if "softmax" in steps:
        sc = dev(s).requires_grad_()
        al = neighbour_softmax(sc, nl)
        al.backward(dev(gs))
        want = M.softmax(s, ent)
        assert same(al, want), "softmax"
        assert same(sc.grad, M.softmax_backward(want, gs, ent)), "softmax gradient"
        assert not al[:, torch.from_numpy(~ent.valid).to(DEV)].any()
    if "sum" in steps:
        xt, wt = dev(a).requires_grad_(), dev(w).requires_grad_()
        y = head_aggregate(xt, nl, wt)
        assert y.shape == xt.shape and y.requires_grad
        y.backward(dev(g))
        assert same(y, M.apply(a, w, ent)), "sum"
        assert same(xt.grad, M.apply_transposed(g, w, ent)) and same(wt.grad, M.dot(g, a, ent, Hd)), "sum gradients"
        if Hd == 1:                                                        # one head: the bits of graph_aggregate and of its gradients
            xa, wa = dev(a).requires_grad_(), dev(w[0]).requires_grad_()
            ya = graph_aggregate(xa, nl, weight=wa)
            ya.backward(dev(g))
            assert same(y, bits(ya).view(F32)) and same(xt.grad, bits(xa.grad).view(F32)) and same(wt.grad[0], bits(wa.grad).view(F32))


def lists_of(frames, K, seed=0):
    nl = neighbour_lists(make_graph(frames, K, DEV, seed))
    return nl, M.Entries(*numpy_lists(nl), len(frames), K)


# ---- graphs, node counts and head widths ----
WIDTHS = [(Hd, D) for Hd in (1, 3) for D in (1, 5, 8, 9, 32, 33)]      # a part of a wave's eight channels, exactly eight, two waves, two blocks


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 257])
def test_paths_and_random_graphs_around_a_wavefront(K):
    rng = np.random.default_rng(K)
    isolated = {0, K - 1} | set(rng.integers(0, K, 5).tolist())
    one = lists_of([path(K) + random_pairs(rng, K, 5)], K)
    # three frames with different edge counts, one of them without an edge; nodes 0 and K - 1 and a few more are isolated
    three = lists_of([random_pairs(rng, K, 6, isolated), [], path(K)], K)
    for i, (Hd, D) in enumerate(WIDTHS):
        check(*one, Hd, D, seed=i, steps=("dot", "sum"))
        check(*three, Hd, D, seed=100 + i, steps=("dot", "sum"))
    for Hd in (1, 3, 5):                                                   # (the softmax sees no channels: heads below, at and above a block's four)
        check(*one, Hd, 1, seed=Hd, steps=("softmax",))
        check(*three, Hd, 1, seed=10 + Hd, steps=("softmax",))


@pytest.mark.parametrize("K,degree", [(400, 300), (1100, 1025)])
def test_star_hubs_longer_than_a_wavefront_and_the_window(K, degree):
    """The hub's row (and, transposed, its target) is walked in full and in order, and the rows behind it in its tile start beyond the
    LDS window."""
    rng = np.random.default_rng(degree)
    check(*lists_of([star(K, degree)], K), 3, 5)
    check(*lists_of([star(K, degree, hub=5) + random_pairs(rng, K, 4), path(K)], K), 1, 9, seed=1)


def test_softmax_edges():
    K = 130
    nl, ent = lists_of([star(K, 100, hub=3) + path(K), path(K)], K)
    rng = np.random.default_rng(2)
    s = rng.uniform(-8, 8, (3, ent.nnz)).astype(F32)
    hub = np.nonzero(ent.rows == 3)[0]
    assert len(hub) >= 100 and ent.valid_degree[0] == 1 and ent.valid_degree[K] == 1
    s[0, hub] = np.linspace(0, -95, len(hub)).astype(F32)                  # the smallest exponentials are subnormal
    s[1, hub] = F32(2.5)                                                   # every entry at the maximum
    s[2, hub[::3]] = -np.inf                                               # -inf beside finite scores
    s[2, hub[1]] = s[2, hub[2]] = F32(7.75)                                # two at the maximum
    want = M.softmax(s, ent)
    tiny = want[0, hub][(want[0, hub] > 0)]
    assert tiny.min() < 2.0 ** -126 and (want[2, hub[::3]] == 0).all() and (want[1, hub] == F32(1) / F32(len(hub))).all()
    single = np.nonzero(np.isin(ent.rows, [0, K]))[0]
    assert (want[:, single] == 1).all()
    check(nl, ent, 3, 1, scores=s, steps=("softmax",))
    sc = dev(s).requires_grad_()
    neighbour_softmax(sc, nl).backward(dev(np.full(s.shape, 3.5, F32)))
    grad = sc.grad.cpu().numpy()
    assert not grad[:, single].any() and not np.signbit(grad[:, single]).any()      # a single entry: alpha = 1 exactly, the gradient +0.0
    # the 1-D form of one head
    one = dev(s[0]).requires_grad_()
    al = neighbour_softmax(one, nl)
    al.backward(dev(s[1]))
    assert tuple(al.shape) == (ent.nnz,) and same(al, want[0]) and same(one.grad, M.softmax_backward(want[:1], s[1:2], ent)[0])
    y = head_aggregate(dev(np.ones((2, 2, K), F32)), nl, al.detach())      # and as the weight of one head
    assert same(y, M.apply(np.ones((2, 2, K), F32), want[:1], ent))


def test_raw_pair_with_invalid_entries():
    """Entries -1 and K, and the entries behind the last row, are +0.0 everywhere and count into nothing."""
    rng = np.random.default_rng(4)
    N, K = 2, 257
    offsets, indices = numpy_lists(neighbour_lists(make_graph([random_pairs(rng, K, 7), random_pairs(rng, K, 5)], K)))
    indices = np.concatenate([indices, rng.integers(0, K, 70).astype(np.int32)])      # 70 entries that no row holds
    bad = rng.random(len(indices)) < 0.2
    indices[bad] = rng.choice([-1, K], bad.sum()).astype(np.int32)
    indices[:3], indices[-1] = (-1, K, -1), K
    ent = M.Entries(offsets, indices, N, K)
    assert (~ent.valid).sum() > 120 and not ent.valid[-70:].any()
    pair = (dev(offsets), dev(indices))
    nl = neighbour_lists(pair, num_frames=N, num_components=K)
    check(nl, ent, 3, 5)
    check(nl, ent, 1, 9, seed=1)
    a, s = rng.standard_normal((N, 6, K)).astype(F32), rng.standard_normal((2, ent.nnz)).astype(F32)
    invalid = torch.from_numpy(~ent.valid).to(DEV)
    for got, want in ((neighbour_dot(dev(a), dev(a), pair, 2), M.dot(a, a, ent, 2)),      # the pair itself: the lists are built by the call
                      (neighbour_softmax(dev(s), pair, num_frames=N, num_components=K), M.softmax(s, ent))):
        assert same(got, want) and not got[:, invalid].any() and not np.signbit(got[:, invalid].cpu().numpy()).any() and got[:, ~invalid].any()
    assert same(head_aggregate(dev(a), pair, dev(s)), M.apply(a, s, ent))


def test_non_contiguous_and_unbatched_tensors():
    rng = np.random.default_rng(3)
    K, Hd, D = 130, 2, 3
    nl, ent = lists_of([random_pairs(rng, K, 6)], K)
    a, b, g = (rng.standard_normal((1, Hd * D, K)).astype(F32) for _ in range(3))
    w, gs = (rng.standard_normal((Hd, ent.nnz)).astype(F32) for _ in range(2))
    leaf = dev(a.transpose(0, 2, 1)).requires_grad_()                      # [1, K, C] in memory
    wleaf = dev(w.T).requires_grad_()                                      # [nnz, Hd] in memory
    xt, wt = leaf.transpose(1, 2), wleaf.T
    assert not xt.is_contiguous() and not wt.is_contiguous()
    y = head_aggregate(xt, nl, wt)
    y.backward(dev(g.transpose(0, 2, 1)).transpose(1, 2))                  # a non-contiguous gradient as well
    assert same(y, M.apply(a, w, ent)) and same(leaf.grad.transpose(1, 2), M.apply_transposed(g, w, ent)) and same(wleaf.grad.T, M.dot(g, a, ent, Hd))
    sleaf = dev(w.T).requires_grad_()
    al = neighbour_softmax(sleaf.T, nl)
    al.backward(dev(gs.T).T)
    assert same(al, M.softmax(w, ent)) and same(sleaf.grad.T, M.softmax_backward(M.softmax(w, ent), gs, ent))
    a2, b2 = dev(a[0]).requires_grad_(), dev(b.transpose(0, 2, 1))[0].T.requires_grad_()      # [C, K], one of them non-contiguous
    s = neighbour_dot(a2, b2, nl, Hd)
    s.backward(dev(gs.T).T)
    assert tuple(s.shape) == (Hd, ent.nnz) and same(s, M.dot(a, b, ent, Hd))
    assert same(a2.grad, M.apply(b, gs, ent)[0]) and same(b2.grad, M.apply_transposed(a, gs, ent)[0])
    y = head_aggregate(a2, nl, dev(w))
    assert tuple(y.shape) == (Hd * D, K) and same(y, M.apply(a, w, ent)[0])
    q2 = dev(a[0])
    y, alpha = graph_attention(q2, dev(b[0]), q2, nl, Hd, return_weights=True)
    want = M.attention(a, b, a, ent, Hd)
    assert tuple(y.shape) == (Hd * D, K) and same(y, want[0][0]) and same(alpha, want[1])


# ---- once round each kernel's loop ----
@pytest.mark.parametrize("Hd,D", [(3, 8 * 841 - 3), (842, 24)])
def test_more_sum_items_than_blocks(Hd, D):
    """13 tiles of 64 rows x 3 * 211 groups of 32 channels of a head = 8229 items, and with heads narrower than 32 channels 13 tiles x
    632 groups of four eight-channel chunks = 8216 items, for the 8192 blocks of a launch."""
    rng = np.random.default_rng(5)
    K = 257
    nl, ent = lists_of([random_pairs(rng, K, 3), [], path(K)], K)
    x = rng.standard_normal((3, Hd * D, K)).astype(F32)
    w = rng.standard_normal((Hd, ent.nnz)).astype(F32)
    xt = dev(x).requires_grad_()
    y = head_aggregate(xt, nl, dev(w))
    y.backward(xt.detach())
    assert same(y, M.apply(x, w, ent)) and same(xt.grad, M.apply_transposed(x, w, ent))


def test_more_rows_and_entries_than_a_launch_holds():
    """Paths of 58300 nodes in 9 frames: 8199 tiles of 64 rows for the softmax's 8192 blocks, and 1049382 entries for the 524288
    threads of the dot."""
    N, K = 9, 58300
    degree = np.full(K, 2, np.int64)
    degree[[0, K - 1]] = 1
    offsets = np.concatenate([[0], np.cumsum(np.tile(degree, N))])
    node = np.arange(K, dtype=np.int32)
    indices = np.tile(np.stack([node - 1, node + 1], 1).ravel()[1:-1], N)
    nl = neighbour_lists((dev(offsets), dev(indices)), num_frames=N, num_components=K)
    ent = M.Entries(offsets, indices, N, K)
    assert ent.valid.all() and (N * K + 63) // 64 > 8192 and ent.nnz > 2048 * 256
    check(nl, ent, 1, 2, steps=("dot", "softmax"))


# ---- the composition ----
@pytest.mark.parametrize("connectivity", [4, 8])
def test_graph_attention_on_the_graph_of_a_label_map(connectivity):
    K, N, Hd, Cc, Cv = 60, 2, 2, 6, 4
    maps = np.stack([connect_ref.blocky(37, 53, K, seed=s) for s in (1, 2)])
    graph = superpixel_graph(dev(maps), K, connectivity)
    nl = neighbour_lists(graph)
    ent = M.Entries(*numpy_lists(nl), N, K)
    rng = np.random.default_rng(connectivity)
    q, k = (rng.standard_normal((N, Cc, K)).astype(F32) for _ in range(2))
    v, gy = (rng.standard_normal((N, Cv, K)).astype(F32) for _ in range(2))
    for scale in (None, 0.3):
        qt, kt, vt = (dev(t).requires_grad_() for t in (q, k, v))
        y, alpha = graph_attention(qt, kt, vt, graph, Hd, scale, return_weights=True)      # the graph itself: the lists are built by the call
        y.backward(dev(gy))
        want_y, want_alpha, grads = M.attention(q, k, v, ent, Hd, scale, gy=gy)
        assert same(y, want_y) and same(alpha, want_alpha)
        assert all(same(t.grad, want) for t, want in zip((qt, kt, vt), grads))
        # and the three calls in sequence give these bits
        s = neighbour_dot(qt.detach() * float(F32(0.3 if scale else (Cc // Hd) ** -0.5)), kt.detach(), nl, Hd)
        assert torch.equal(head_aggregate(vt.detach(), nl, neighbour_softmax(s, nl)).view(torch.int32), y.detach().view(torch.int32))
        # within the bound of the float64 dense attention (tests/attention_ref.py, as on the CPU)
        y64, alpha64, bound = M.attention_bound(q, k, v, ent, Hd, scale)
        assert (np.abs(y.detach().cpu().numpy() - y64) <= bound).all() and np.abs(y64).max() > 0.1


def test_the_same_bits_from_run_to_run():
    rng = np.random.default_rng(7)
    N, K, Hd, Cc = 3, 1600, 4, 32
    nl, ent = lists_of([random_pairs(rng, K, 6) + star(K, 700) for _ in range(N)], K)
    q, k, v, gy = (dev(rng.standard_normal((N, Cc, K)).astype(F32)) for _ in range(4))

    def run():
        leaves = [t.clone().requires_grad_() for t in (q, k, v)]
        y = graph_attention(*leaves, nl, Hd)
        y.backward(gy)
        return [y.detach()] + [t.grad for t in leaves]

    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(run(), run()))


def test_side_stream_and_no_host_synchronisation():
    """The three steps and graph_attention, of lists, of a graph and of a raw pair, and every backward, on a stream of the caller's
    and with torch refusing every host synchronisation: the bits of the plain call."""
    rng = np.random.default_rng(9)
    N, K, Hd, Cc = 2, 300, 2, 6
    g = make_graph([random_pairs(rng, K, 6), random_pairs(rng, K, 4)], K, DEV)
    q, k, v, gy = (dev(rng.standard_normal((N, Cc, K)).astype(F32)) for _ in range(4))
    gs = dev(rng.standard_normal((Hd, 2 * g.edge_index.shape[1])).astype(F32))

    def calls():
        nl = neighbour_lists(g)
        qt, kt, vt = (t.clone().requires_grad_() for t in (q, k, v))
        y, alpha = graph_attention(qt, kt, vt, g, Hd, return_weights=True)
        y.backward(gy)
        a, b = q.clone().requires_grad_(), k.clone().requires_grad_()
        s = neighbour_dot(a, b, (nl.offsets, nl.indices), Hd)
        s.backward(gs)
        sc = gs.clone().requires_grad_()
        al = neighbour_softmax(sc, nl)
        al.backward(gs)
        return y.detach(), alpha.detach(), qt.grad, kt.grad, vt.grad, s.detach(), a.grad, b.grad, al.detach(), sc.grad

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
        assert other is None or all(np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8)) for a, b in zip(want, other))
