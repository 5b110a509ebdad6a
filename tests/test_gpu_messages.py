"""Messages over neighbour lists on the MI355X (fast_slic_amd/messages.py, csrc/message.hip) against the model written from the rules
(tests/messages_ref.py), with exact equality throughout: both gathers and the four reductions in both directions, each forward and
every gradient, on paths, random graphs with isolated nodes and a frame without an edge at node counts around a wavefront, feature
counts around the four waves of a reduce block, stars whose hub is longer than a wavefront and than the LDS window, extrema with ties
and infinities, a raw pair with invalid entries and one with garbage offsets, knn_graph's padded lists, non-contiguous, unbatched and
1-D tensors, the three identities with graph_aggregate and head_aggregate, the same bits from run to run, a side stream without host
synchronisation."""
import numpy as np
import pytest
import torch

import messages_ref as R
from fast_slic_amd.attention import head_aggregate
from fast_slic_amd.knn import knn_graph
from fast_slic_amd.messages import entry_gather, entry_reduce
from fast_slic_amd.propagate import graph_aggregate, neighbour_lists
from test_aggregate_cpu import make_graph, numpy_lists, path, random_pairs, star

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
ENDS = ("target", "source")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(got, want):
    return tuple(got.shape) == tuple(np.shape(want)) and np.array_equal(bits(got), bits(want))


def same_int(got, want):
    return got.dtype == torch.int32 and tuple(got.shape) == tuple(want.shape) and np.array_equal(got.cpu().numpy(), want)


def lists_of(frames, K, seed=0):
    nl = neighbour_lists(make_graph(frames, K, DEV, seed))
    return nl, R.Entries(*numpy_lists(nl), len(frames), K)


def check_gathers(nl, ent, C, seed=0):
    """Both gathers of C channels on `nl` (NeighbourLists on the GPU; ent the same lists for the model), forward and gradient."""
    rng = np.random.default_rng(seed)
    x, g = rng.standard_normal((ent.N, C, ent.K)).astype(F32), rng.standard_normal((C, ent.nnz)).astype(F32)
    invalid = torch.from_numpy(~ent.valid).to(DEV)
    for end in ENDS:
        xt = dev(x).requires_grad_()
        out = entry_gather(xt, nl, end)
        assert out.dtype == torch.float32 and out.device == DEV and out.requires_grad
        out.backward(dev(g))
        assert same(out, R.gather(x, ent, end)), end
        assert same(xt.grad, R.gather_backward(g, ent, end)), end
        assert not out[:, invalid].any() and not np.signbit(out[:, invalid].detach().cpu().numpy()).any()
        with torch.no_grad():                                              # outside autograd: the same launch, the same bits
            assert torch.equal(entry_gather(xt, nl, end).view(torch.int32), out.detach().view(torch.int32))


def check_reduces(nl, ent, Fc, seed=0, m=None, hows=R.REDUCES):
    """The reductions of Fc features in both directions, forward, argmax and gradient."""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((Fc, ent.nnz)).astype(F32) if m is None else m
    g = rng.standard_normal((ent.N, Fc, ent.K)).astype(F32)
    invalid = torch.from_numpy(~ent.valid).to(DEV)
    for to in ENDS:
        for how in hows:
            mt = dev(m).requires_grad_()
            extremum = how in ("max", "min")
            res = entry_reduce(mt, nl, how, to, return_argmax=extremum)
            y, arg = res if extremum else (res, None)
            assert y.dtype == torch.float32 and tuple(y.shape) == (ent.N, Fc, ent.K) and y.requires_grad
            y.backward(dev(g))
            want_y, want_arg, deg = R.reduce(m, ent, how, to)
            assert same(y, want_y), (how, to)
            assert arg is None or (same_int(arg, want_arg) and not arg.requires_grad), (how, to)
            assert same(mt.grad, R.reduce_backward(g, ent, how, to, want_arg, deg)), (how, to)
            assert not mt.grad[:, invalid].any() and not np.signbit(mt.grad[:, invalid].cpu().numpy()).any()
            empty = torch.from_numpy((deg == 0).reshape(ent.N, 1, ent.K)).to(DEV).expand_as(y)
            assert not y[empty].any() and not np.signbit(y[empty].detach().cpu().numpy()).any() and (arg is None or (arg[empty] == -1).all())
            with torch.no_grad():
                assert torch.equal(entry_reduce(mt, nl, how, to).view(torch.int32), y.detach().view(torch.int32))


# ---- graphs, node counts, channels and features ----
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 257])
def test_paths_and_random_graphs_around_a_wavefront(K):
    rng = np.random.default_rng(K)
    isolated = {0, K - 1} | set(rng.integers(0, K, 5).tolist())
    one = lists_of([path(K) + random_pairs(rng, K, 5)], K)
    # three frames with different edge counts, one of them without an edge; nodes 0 and K - 1 and a few more are isolated
    three = lists_of([random_pairs(rng, K, 6, isolated), [], path(K)], K)
    for i, C in enumerate((1, 8, 33)):
        check_gathers(*one, C, seed=i)
        check_gathers(*three, C, seed=10 + i)
    for Fc in (1, 3, 4, 5):                                                # the waves of a reduce block: below, at and above four
        check_reduces(*one, Fc, seed=Fc)
        check_reduces(*three, Fc, seed=10 + Fc)


@pytest.mark.parametrize("K,degree", [(400, 300), (1100, 1025)])
def test_star_hubs_longer_than_a_wavefront_and_the_window(K, degree):
    """The hub's row (and, transposed, its target) is walked in full and in order; with the hub at node 5 the rows behind it in its
    tile start beyond the LDS window."""
    rng = np.random.default_rng(degree)
    nl, ent = lists_of([star(K, degree, hub=5) + random_pairs(rng, K, 2), path(K)], K)
    assert ent.valid_degree[5] >= degree and ent.begin[6] - ent.begin[0] >= degree
    check_gathers(nl, ent, 3)
    check_reduces(nl, ent, 3, seed=1)
    check_reduces(*lists_of([star(K, degree)], K), 5, seed=2, hows=("sum", "max"))


def test_extrema_with_ties_and_infinities():
    K = 130
    nl, ent = lists_of([star(K, 100, hub=3) + path(K), path(K) + random_pairs(np.random.default_rng(1), K, 6)], K)
    rng = np.random.default_rng(2)
    m = rng.integers(-2, 3, (3, ent.nnz)).astype(F32)                      # five values: ties in every row of two entries or more
    hub = np.nonzero(ent.rows == 3)[0]
    m[1, hub] = F32(2.5)                                                   # every entry of the hub at the extremum: the first one wins
    m[2, hub[::3]], m[2, hub[1::3]] = np.inf, -np.inf                      # +inf and -inf beside finite values
    m[2, np.nonzero(ent.rows == 0)[0]] = -np.inf                           # a single entry, -inf: it is the maximum
    want = R.reduce(m, ent, "max", "target")
    assert (want[1][0, 1, 3] == hub[0]) and want[0][0, 2, 3] == np.inf and want[0][0, 2, 0] == -np.inf and want[1][0, 2, 0] >= 0
    assert R.reduce(m, ent, "min", "target")[0][0, 2, 3] == -np.inf
    check_reduces(nl, ent, 3, m=m, hows=("max", "min"))
    for how in ("max", "min"):                                             # a gradient of +inf goes to the argmax and to nothing else
        mt = dev(m).requires_grad_()
        y = entry_reduce(mt, nl, how)
        y.backward(torch.full_like(y, float("inf")))
        assert same(mt.grad, R.reduce_backward(np.full(tuple(y.shape), np.inf, F32), ent, how, "target", R.reduce(m, ent, how)[1]))
        assert not torch.isnan(mt.grad).any() and (mt.grad == float("inf")).sum() == (R.reduce(m, ent, how)[2] > 0).sum() * 3


# ---- lists that are not a graph's ----
def test_raw_pair_with_invalid_entries():
    """Entries -1 and K, and the entries behind the last row, are +0.0 everywhere and count into nothing."""
    rng = np.random.default_rng(4)
    N, K = 2, 257
    offsets, indices = numpy_lists(neighbour_lists(make_graph([random_pairs(rng, K, 7), random_pairs(rng, K, 5)], K)))
    indices = np.concatenate([indices, rng.integers(0, K, 70).astype(np.int32)])      # 70 entries that no row holds
    bad = rng.random(len(indices)) < 0.2
    indices[bad] = rng.choice([-1, K], bad.sum()).astype(np.int32)
    indices[:3], indices[-1] = (-1, K, -1), K
    ent = R.Entries(offsets, indices, N, K)
    assert (~ent.valid).sum() > 120 and not ent.valid[-70:].any()
    pair = (dev(offsets), dev(indices))
    nl = neighbour_lists(pair, num_frames=N, num_components=K)
    check_gathers(nl, ent, 5)
    check_reduces(nl, ent, 3, seed=1)
    x, m = rng.standard_normal((N, 2, K)).astype(F32), rng.standard_normal((2, ent.nnz)).astype(F32)
    assert same(entry_gather(dev(x), pair, "source"), R.gather(x, ent, "source"))      # the pair itself: the lists are built by the call
    assert same(entry_reduce(dev(m), pair, "mean", "source", num_frames=N, num_components=K), R.reduce(m, ent, "mean", "source")[0])


def test_garbage_offsets_are_clamped():
    """An end before its start, a negative offset and offsets beyond nnz: the reduce over the rows is still what the clamped bounds
    say, row by row, and everything else only has to run without a fault."""
    rng = np.random.default_rng(6)
    K, Fc = 130, 3
    offsets, indices = numpy_lists(neighbour_lists(make_graph([path(K) + random_pairs(rng, K, 6)], K)))
    nnz = len(indices)
    indices = indices.copy()
    indices[rng.random(nnz) < 0.1] = -1
    bad = offsets.copy()
    bad[21] = bad[20] - 3                                                  # row 20 ends before it starts; row 21 starts three entries early
    bad[5] = -7                                                            # row 4 is empty, row 5 starts at 0
    bad[-3:] += nnz + 1000                                                 # the last row but two runs to nnz, the last two are empty
    m = rng.standard_normal((Fc, nnz)).astype(F32)
    want, want_max, want_arg = np.zeros((1, Fc, K), F32), np.zeros((1, Fc, K), F32), np.full((1, Fc, K), -1, np.int32)
    for r in range(K):
        acc, best = np.zeros(Fc, F32), None
        for p in range(int(np.clip(bad[r], 0, nnz)), int(np.clip(bad[r + 1], 0, nnz))):
            if 0 <= indices[p] < K:
                acc = acc + m[:, p]
                take = np.ones(Fc, bool) if best is None else m[:, p] > best
                best = np.where(take, m[:, p], best if best is not None else 0).astype(F32)
                want_arg[0, :, r] = np.where(take, p, want_arg[0, :, r])
        want[0, :, r] = acc
        want_max[0, :, r] = 0 if best is None else best
    assert not want[0, :, [4, 20, K - 2, K - 1]].any() and want[0, :, 5].any() and want[0, :, 21].any()
    pair = (dev(bad), dev(indices))
    assert same(entry_reduce(dev(m), pair, num_frames=1, num_components=K), want)
    y, arg = entry_reduce(dev(m), pair, "max", return_argmax=True, num_frames=1, num_components=K)
    assert same(y, want_max) and same_int(arg, want_arg)
    # no fault: the rows of the entries and the transposed lists are built from these offsets and are garbage themselves
    nl = neighbour_lists(pair, num_frames=1, num_components=K)
    x = dev(rng.standard_normal((1, Fc, K)).astype(F32)).requires_grad_()
    for end in ENDS:
        for how in R.REDUCES:
            mt = dev(m).requires_grad_()
            out = entry_reduce(mt * entry_gather(x, nl, end), nl, how, end)
            out.sum().backward()
            assert tuple(out.shape) == (1, Fc, K) and tuple(mt.grad.shape) == (Fc, nnz)
    torch.cuda.synchronize()


def test_knn_graph_lists_with_padding():
    rng = np.random.default_rng(8)
    N, K, k = 2, 70, 16
    pts = dev(rng.standard_normal((N, 4, K)).astype(F32))
    valid = torch.ones((N, K), dtype=torch.bool, device=DEV)
    valid[1, 9:] = False                                                   # nine valid nodes in frame 1: rows of eight neighbours and padding
    nl, _ = knn_graph(pts, k, valid=valid)
    ent = R.Entries(*numpy_lists(nl), N, K)
    assert ent.nnz == N * K * k and (~ent.valid).sum() == K * k - 9 * 8
    check_gathers(nl, ent, 4)
    check_reduces(nl, ent, 2, seed=1)


def test_non_contiguous_unbatched_and_one_dimensional_tensors():
    rng = np.random.default_rng(3)
    K, C = 130, 3
    nl, ent = lists_of([random_pairs(rng, K, 6)], K)
    x, gy = (rng.standard_normal((1, C, K)).astype(F32) for _ in range(2))
    m, gm = (rng.standard_normal((C, ent.nnz)).astype(F32) for _ in range(2))
    leaf = dev(x.transpose(0, 2, 1)).requires_grad_()                      # [1, K, C] in memory
    xt = leaf.transpose(1, 2)
    assert not xt.is_contiguous()
    out = entry_gather(xt, nl, "source")
    out.backward(dev(gm.T).T)                                              # a non-contiguous gradient as well
    assert same(out, R.gather(x, ent, "source")) and same(leaf.grad.transpose(1, 2), R.gather_backward(gm, ent, "source"))
    mleaf = dev(m.T).requires_grad_()                                      # [nnz, F] in memory
    y = entry_reduce(mleaf.T, nl, "mean")
    y.backward(dev(gy.transpose(0, 2, 1)).transpose(1, 2))
    want, _, deg = R.reduce(m, ent, "mean")
    assert same(y, want) and same(mleaf.grad.T, R.reduce_backward(gy, ent, "mean", "target", None, deg))
    x2 = dev(x[0]).requires_grad_()                                        # [C, K]
    out = entry_gather(x2, nl)
    out.backward(dev(gm))
    assert tuple(out.shape) == (C, ent.nnz) and same(out, R.gather(x, ent, "target")) and same(x2.grad, R.gather_backward(gm, ent, "target")[0])
    m1 = dev(m[0]).requires_grad_()                                        # [nnz]: one feature
    y, arg = entry_reduce(m1, nl, "min", "source", return_argmax=True)
    y.backward(dev(gy[:, :1]))
    want, want_arg, _ = R.reduce(m[:1], ent, "min", "source")
    assert tuple(y.shape) == (1, 1, K) and same(y, want) and same_int(arg, want_arg)
    assert tuple(m1.grad.shape) == (ent.nnz,) and same(m1.grad, R.reduce_backward(gy[:, :1], ent, "min", "source", want_arg)[0])


# ---- the identities with graph_aggregate and head_aggregate, on the GPU ----
def test_identities_with_graph_aggregate_and_head_aggregate():
    rng = np.random.default_rng(5)
    N, K, C = 2, 257, 9
    nl, ent = lists_of([random_pairs(rng, K, 6) + star(K, 80, hub=7), path(K)], K)
    x, g = (dev(rng.standard_normal((N, C, K)).astype(F32)) for _ in range(2))
    x[0, 0, : K // 2] = 0.5                                                # ties for the max
    w = dev(rng.standard_normal(ent.nnz).astype(F32))
    eq = lambda a, b: a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    for how in ("sum", "mean", "max"):
        xa, xm = x.clone().requires_grad_(), x.clone().requires_grad_()
        ya = graph_aggregate(xa, nl, reduce=how, return_argmax=how == "max")
        ym = entry_reduce(entry_gather(xm, nl, "source"), nl, how, return_argmax=how == "max")
        if how == "max":
            assert torch.equal(ya[1], ym[1])
            ya, ym = ya[0], ym[0]
        ya.backward(g)
        ym.backward(g)
        assert eq(ya, ym) and eq(xa.grad, xm.grad), how
    # the weighted sum: y and grad_x bit for bit; grad_w through the left fold over c of grad_m * x_j, as graph_aggregate folds it
    xa, wa, xm = x.clone().requires_grad_(), w.clone().requires_grad_(), x.clone().requires_grad_()
    ya = graph_aggregate(xa, nl, weight=wa)
    xj = entry_gather(xm, nl, "source")
    msg = w[None] * xj
    msg.retain_grad()
    ym = entry_reduce(msg, nl)
    ya.backward(g)
    ym.backward(g)
    assert eq(ya, ym) and eq(xa.grad, xm.grad)
    gm, xjn = msg.grad.cpu().numpy(), xj.detach().cpu().numpy()
    acc = np.zeros(ent.nnz, F32)
    for c in range(C):
        acc = acc + gm[c] * xjn[c]
    assert same(wa.grad, acc)
    # the sum to the source is head_aggregate's gradient for the values with g = 1 (rule A transposed), one head a feature
    m = dev(rng.standard_normal((C, ent.nnz)).astype(F32))
    v = torch.zeros((N, C, K), device=DEV).requires_grad_()
    head_aggregate(v, nl, m).backward(torch.ones((N, C, K), device=DEV))
    assert eq(entry_reduce(m, nl, "sum", "source"), v.grad)


# ---- the same bits, whatever runs beside ----
def layer(x, w, nl):
    """An EdgeConv with a PNA tail, the message elementwise (no matrix product of torch's): every function and every gradient of the
    module in one graph."""
    xi, xj = entry_gather(x, nl, "target"), entry_gather(x, nl, "source")
    m = torch.relu(w[0] * xi + w[1] * (xj - xi))
    return torch.cat([entry_reduce(m, nl, how, to) for how in R.REDUCES for to in ENDS], 1)


def test_the_same_bits_from_run_to_run():
    rng = np.random.default_rng(7)
    N, K, C = 3, 1600, 8
    nl, _ = lists_of([random_pairs(rng, K, 6) + star(K, 700) for _ in range(N)], K)
    x, w = dev(rng.standard_normal((N, C, K)).astype(F32)), dev(rng.standard_normal((2, C, 1)).astype(F32))
    gy = dev(rng.standard_normal((N, 8 * C, K)).astype(F32))

    def run():
        xt = x.clone().requires_grad_()
        y = layer(xt, w, nl)
        y.backward(gy)
        return y.detach(), xt.grad

    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(run(), run()))


def test_side_stream_and_no_host_synchronisation():
    """Every function of lists, of a graph and of a raw pair, and every backward, on a stream of the caller's and with torch refusing
    every host synchronisation: the bits of the plain call."""
    rng = np.random.default_rng(9)
    N, K, C = 2, 300, 4
    g = make_graph([random_pairs(rng, K, 6), random_pairs(rng, K, 4)], K, DEV)
    x, w = dev(rng.standard_normal((N, C, K)).astype(F32)), dev(rng.standard_normal((2, C, 1)).astype(F32))
    gy = dev(rng.standard_normal((N, 8 * C, K)).astype(F32))
    m = dev(rng.standard_normal((C, 2 * g.edge_index.shape[1])).astype(F32))

    def calls():
        nl = neighbour_lists(g)
        xt = x.clone().requires_grad_()
        y = layer(xt, w, nl)
        y.backward(gy)
        a = entry_gather(x, g, "source")
        b, arg = entry_reduce(m, (nl.offsets, nl.indices), "max", "source", return_argmax=True, num_frames=N, num_components=K)
        return y.detach(), xt.grad, a, b, arg

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
