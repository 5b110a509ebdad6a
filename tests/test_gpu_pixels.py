"""Pixels over neighbour lists on the MI355X (fast_slic_amd/pixels.py, csrc/pixel.hip) against the model written from the rules
(tests/pixels_ref.py).  Dot, softmax, mix and every gradient that is one of them: exact bit equality, +0.0 on every empty slot.  The
scatter and the three gradients that are scatters: exact bits on inputs built so that no tile partial rounds (small integers times
powers of two, from 2^-100 to 2^100, and x / -x pairs that cancel), the bits of superpixel_pool's sum at S = 1 with unit weights, and on
random normal inputs the float64 sum within gamma(1026) * sum |w x| (pixels_ref's docstring derives it).  Frames of one pixel, one exact
tile, four tiles with one-pixel remainders and more; K from 1 to 70, S in {1, 2, 9, 32}, C in {1, 3, 8} with 1, 2 and 4 heads, one and
three frames; int16 maps with -1, int32 and int64 maps with labels beyond K; random lists with empty rows, a hub that is cut, knn_graph's
padded lists, a raw pair with garbage offsets, one label over the whole frame.  The same bits from run to run and at another batch
position, non-contiguous and unbatched inputs, a side stream without host synchronisation, pixel_attention against its composition, and
the peak memory of a scatter."""
import ctypes as C

import numpy as np
import pytest
import torch

import pixels_ref as R
from fast_slic_amd import _binding as B
from fast_slic_amd.knn import knn_graph
from fast_slic_amd.pixels import pixel_attention, pixel_dot, pixel_mix, pixel_scatter, pixel_slots, pixel_softmax
from fast_slic_amd.pool import superpixel_pool
from fast_slic_amd.propagate import neighbour_lists
from test_aggregate_cpu import make_graph, numpy_lists, path, random_pairs, star

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
LABEL_TYPES = {"int16": np.int16, "int32": np.int32, "int64": np.int64}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(got, want):
    return tuple(got.shape) == tuple(np.shape(want)) and np.array_equal(bits(got), bits(want))


def positive_zeros(t, where):
    a = t.detach().cpu().numpy()[where]
    return not a.any() and not np.signbit(a).any()


def within(got, x, w, sl, K):
    """The scatter of random inputs against the float64 sum: gamma(1026) * sum |w x|."""
    want, mag = R.scatter_sum64(x, w, sl, K)
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - want)
    print("scatter: largest error / bound = %.3g" % (err / np.maximum(R.scatter_bound(mag), 1e-300)).max())
    return tuple(got.shape) == want.shape and (err <= R.scatter_bound(mag)).all()


def random_map(rng, N, H, W, K, kind, blocks=False):
    """A map of the label type `kind`: per-pixel random labels (a tile then holds up to K distinct ones) or blocks of 5 x 11 pixels,
    with -1 (int16) or labels from K on (int32, int64) among them."""
    lo, hi = (-1, K) if kind == "int16" else (0, K + 2)
    if blocks:
        coarse = rng.integers(lo, hi, (N, (H + 4) // 5, (W + 10) // 11))
        labels = np.repeat(np.repeat(coarse, 5, axis=1), 11, axis=2)[:, :H, :W]
    else:
        labels = rng.integers(lo, hi, (N, H, W))
    return np.ascontiguousarray(labels.astype(LABEL_TYPES[kind]))


def exact_inputs(rng, labels, sl, C_, Hd, K):
    """x = a small integer times a power of two that depends on the pixel's label and the channel, w = a small integer times a power
    of two that depends on the head and the slot: the products of one (label, slot, channel) share their exponent and their sums stay
    below 2^15 units, so no order of adding a tile's products rounds.  The exponents of the products reach from -100 to 100."""
    N, S = sl.shape[:2]
    ex = rng.integers(-60, 61, (N, K + 1, C_))
    ex[:, 0, 0], ex[:, min(1, K - 1), C_ - 1] = -60, 60
    lab = np.where((labels >= 0) & (labels < K), labels, K).astype(np.int64)
    e_px = np.moveaxis(ex[np.arange(N).reshape(N, 1, 1), lab], -1, 1)                     # [N, C, H, W]
    x = np.ldexp(rng.integers(-8, 9, e_px.shape).astype(np.float64), e_px).astype(F32)
    ew = rng.integers(-40, 41, (N, Hd, S))
    ew[:, 0, 0], ew[:, Hd - 1, S - 1] = -40, 40
    w = np.ldexp(rng.integers(1, 5, (N, Hd, S) + labels.shape[1:]).astype(np.float64), ew[:, :, :, None, None]).astype(F32)
    return x, w


def check_all(nl, offsets, indices, labels, K, S, C_, Hd, seed=0):
    """Every function and every gradient on one map and one set of lists (nl on the GPU; offsets and indices the same for the model)."""
    rng = np.random.default_rng(seed)
    N, H, W = labels.shape
    sl = R.slots(labels, offsets, indices, N, K, S)
    empty = np.broadcast_to((sl < 0)[:, None], (N, Hd, S, H, W))
    lab = dev(labels)
    got = pixel_slots(lab, nl, S)
    assert got.dtype == torch.int32 and got.device == DEV and np.array_equal(got.cpu().numpy(), sl)
    a, x, gp = (rng.standard_normal((N, C_, H, W)).astype(F32) for _ in range(3))
    b, v, gk = (rng.standard_normal((N, C_, K)).astype(F32) for _ in range(3))
    w, gs = (rng.standard_normal((N, Hd, S, H, W)).astype(F32) for _ in range(2))
    # the dot; its gradients are a mix and a scatter
    at, bt = dev(a).requires_grad_(), dev(b).requires_grad_()
    s = pixel_dot(at, bt, lab, nl, S, Hd)
    assert s.dtype == torch.float32 and s.device == DEV and s.requires_grad
    s.backward(dev(gs))
    assert same(s, R.dot(a, b, sl, Hd)) and positive_zeros(s, empty)
    assert same(at.grad, R.mix(b, gs, sl)) and within(bt.grad, a, gs, sl, K)
    with torch.no_grad():                                                      # outside autograd: the same launch, the same bits
        assert torch.equal(pixel_dot(at, bt, lab, nl, S, Hd).view(torch.int32), s.detach().view(torch.int32))
    # the softmax and its backward, from the alpha it returned
    st = dev(w).requires_grad_()
    alpha = pixel_softmax(st, lab, nl)
    alpha.backward(dev(gs))
    want = R.softmax(w, sl)
    assert same(alpha, want) and positive_zeros(alpha, empty)
    assert same(st.grad, R.softmax_backward(want, gs, sl)) and positive_zeros(st.grad, empty)
    # the mix; its gradients are a scatter and a dot
    vt, wt = dev(v).requires_grad_(), dev(w).requires_grad_()
    y = pixel_mix(vt, wt, lab, nl)
    y.backward(dev(gp))
    assert same(y, R.mix(v, w, sl))
    assert within(vt.grad, gp, w, sl, K) and same(wt.grad, R.dot(gp, v, sl, Hd)) and positive_zeros(wt.grad, empty)
    # the scatter; its gradients are a mix and a dot
    xt, wt = dev(x).requires_grad_(), dev(w).requires_grad_()
    z = pixel_scatter(xt, wt, lab, nl, K)
    z.backward(dev(gk))
    assert within(z, x, w, sl, K)
    assert same(xt.grad, R.mix(gk, w, sl)) and same(wt.grad, R.dot(x, gk, sl, Hd)) and positive_zeros(wt.grad, empty)
    # the scatter and the three gradients that are scatters, exactly
    xe, we = exact_inputs(rng, labels, sl, C_, Hd, K)
    want = R.scatter_exact(xe, we, labels, sl, K)
    assert np.array_equal(bits(pixel_scatter(dev(xe), dev(we), lab, nl, K)), want)
    bt = dev(b).requires_grad_()
    pixel_dot(dev(xe), bt, lab, nl, S, Hd).backward(dev(we))
    vt = dev(v).requires_grad_()
    pixel_mix(vt, dev(we), lab, nl).backward(dev(xe))
    assert np.array_equal(bits(bt.grad), want) and np.array_equal(bits(vt.grad), want)
    # S = 1 with unit weights: superpixel_pool's sum
    if S == 1:
        ones = torch.ones((N, Hd, 1, H, W), device=DEV)
        assert torch.equal(pixel_scatter(dev(xe), ones, lab, nl, K).view(torch.int32),
                           superpixel_pool(dev(xe), lab, K, reduce="sum").view(torch.int32))


def lists_of(frames, K, seed=0):
    nl = neighbour_lists(make_graph(frames, K, DEV, seed))
    return (nl,) + numpy_lists(nl)


# name: N, H, W, K, S, C, Hd, label type, blocks
CASES = {
    "one-pixel": (1, 1, 1, 1, 1, 1, 1, "int16", False),
    "one-pixel-two-slots": (1, 1, 1, 2, 2, 1, 1, "int32", False),
    "one-tile": (1, 16, 64, 7, 2, 3, 1, "int32", False),
    "one-tile-pool": (3, 16, 64, 70, 1, 8, 4, "int16", False),
    "four-tiles": (3, 17, 65, 33, 9, 8, 2, "int16", True),
    "hub-cut": (1, 19, 70, 70, 32, 8, 4, "int64", False),
    "blocks": (3, 33, 129, 64, 9, 3, 1, "int32", True),
    "heads-are-channels": (1, 19, 70, 9, 2, 8, 8, "int64", True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_every_function_and_gradient_against_the_model(name):
    N, H, W, K, S, C_, Hd, kind, blocks = CASES[name]
    rng = np.random.default_rng(len(name))
    if name == "hub-cut":                                                      # a hub of 40 neighbours: cut after its first 31
        frames = [path(K) + star(K, 40)]
    elif name == "one-pixel-two-slots":
        frames = [path(K)]
    else:                                                                      # isolated nodes: empty rows; the last frame without an edge
        frames = [random_pairs(rng, K, 6, isolated=(0, K // 2)) for _ in range(N - 1)] + [[]]
        if N == 1:
            frames = [random_pairs(rng, K, 6, isolated=(K - 1,))]
    nl, offsets, indices = lists_of(frames, K)
    if name == "hub-cut":
        assert (np.diff(offsets) > 31).any()
    labels = random_map(rng, N, H, W, K, kind, blocks)
    if H * W == 1:
        labels[:] = K - 1                                                      # the one pixel has a label
    check_all(nl, offsets, indices, labels, K, S, C_, Hd, seed=1)


def test_knn_graph_lists_with_padding():
    rng = np.random.default_rng(8)
    N, K, k = 2, 70, 16
    pts = dev(rng.standard_normal((N, 4, K)).astype(F32))
    valid = torch.ones((N, K), dtype=torch.bool, device=DEV)
    valid[1, 9:] = False                                                       # nine valid nodes in frame 1: rows of eight neighbours and padding
    nl, _ = knn_graph(pts, k, valid=valid)
    offsets, indices = numpy_lists(nl)
    assert (indices < 0).any()
    labels = random_map(rng, N, 19, 70, K, "int16")
    check_all(nl, offsets, indices, labels, K, 9, 3, 1, seed=2)                # the nearest eight of sixteen
    check_all(nl, offsets, indices, labels, K, 32, 8, 2, seed=3)               # all sixteen, and fifteen slots that no pixel fills


def test_garbage_offsets_are_clamped():
    """An end before its start, a negative offset and offsets beyond nnz: the slots are what the clamped bounds say (the terms define
    them for any offsets), so the model still holds; above all nothing faults."""
    rng = np.random.default_rng(6)
    K = 40
    _, offsets, indices = lists_of([path(K) + random_pairs(rng, K, 6)], K)
    bad = offsets.copy()
    bad[3], bad[7], bad[11], bad[20], bad[K] = -5, len(indices) + 1000, 1 << 40, -(1 << 40), 3
    indices = indices.copy()
    indices[::7] = np.array([-1, K, 1 << 30, -(1 << 31)], np.int64).astype(np.int32)[np.arange(len(indices[::7])) % 4]
    pair = (dev(bad), dev(indices))
    labels = random_map(rng, 1, 17, 65, K, "int32")
    check_all(neighbour_lists(pair, 1, K), bad, indices, labels, K, 9, 3, 1, seed=4)
    sl = R.slots(labels, bad, indices, 1, K, 9)
    a, b = rng.standard_normal((1, 3, 17, 65)).astype(F32), rng.standard_normal((1, 3, K)).astype(F32)
    assert same(pixel_dot(dev(a), dev(b), dev(labels), pair, 9), R.dot(a, b, sl, 1))      # the pair itself: the lists are built by the call
    w = rng.standard_normal((1, 1, 9, 17, 65)).astype(F32)
    assert same(pixel_softmax(dev(w), dev(labels), pair, num_components=K), R.softmax(w, sl))


def test_one_label_over_the_whole_frame_and_partials_that_cancel():
    """Every partial of every tile goes onto one node a slot; the right half of the frame holds the left half negated, tile by tile,
    so every total is +0.0 although no partial is."""
    rng = np.random.default_rng(7)
    K, S, C_, Hd, H, W = 3, 2, 3, 1, 16, 128
    nl, offsets, indices = lists_of([path(K)], K)
    labels = np.full((1, H, W), 1, np.int16)
    sl = R.slots(labels, offsets, indices, 1, K, S)
    x, w = exact_inputs(rng, labels, sl, C_, Hd, K)
    x = np.where(x == 0, np.abs(x).max(axis=(2, 3), keepdims=True), np.abs(x))       # every partial is positive; one exponent a channel
    x[..., 64:], w[..., 64:] = -x[..., :64], w[..., :64]
    z = pixel_scatter(dev(x), dev(w), dev(labels), nl, K)
    assert not bits(z).any()                                                   # +0.0 everywhere: nodes 1 and 0 cancel, node 2 is in no slot
    x[..., 64:] = x[..., :64]
    z = pixel_scatter(dev(x), dev(w), dev(labels), nl, K)
    assert np.array_equal(bits(z), R.scatter_exact(x, w, labels, sl, K)) and z[0, :, :2].abs().min() > 0 and not bits(z[0, :, 2]).any()
    nl, offsets, indices = lists_of([path(K), path(K)], K)
    check_all(nl, offsets, indices, np.full((2, 33, 129), 2, np.int32), K, 2, 1, 1, seed=5)


def test_the_same_bits_from_run_to_run_and_at_another_batch_position():
    rng = np.random.default_rng(10)
    N, H, W, K, S, C_, Hd = 3, 33, 129, 50, 9, 8, 2
    frame = random_pairs(rng, K, 6)
    nl, _, _ = lists_of([frame, random_pairs(rng, K, 5), frame], K)
    labels = random_map(rng, N, H, W, K, "int16", blocks=True)
    labels[2] = labels[0]
    x, w = rng.standard_normal((N, C_, H, W)).astype(F32), rng.standard_normal((N, Hd, S, H, W)).astype(F32)
    b = rng.standard_normal((N, C_, K)).astype(F32)
    x[2], w[2], b[2] = x[0], w[0], b[0]
    lab = dev(labels)

    def calls():
        xt, wt, bt = dev(x).requires_grad_(), dev(w).requires_grad_(), dev(b).requires_grad_()
        z = pixel_scatter(xt, wt, lab, nl, K)
        y = pixel_attention(xt, bt, z, lab, nl, S, Hd)
        y.sum().backward()
        return z.detach(), y.detach(), xt.grad, wt.grad, bt.grad

    first, second = calls(), calls()
    for p, q in zip(first, second):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))
        assert torch.equal(p[0].view(torch.int32), p[2].view(torch.int32)) and not torch.equal(p[0], p[1])


def test_non_contiguous_and_unbatched_inputs():
    rng = np.random.default_rng(11)
    H, W, K, S, C_, Hd = 17, 65, 20, 4, 4, 2
    nl, offsets, indices = lists_of([random_pairs(rng, K, 5)], K)
    labels = random_map(rng, 1, H, W, K, "int16")
    sl = R.slots(labels, offsets, indices, 1, K, S)
    x, b = rng.standard_normal((1, C_, H, W)).astype(F32), rng.standard_normal((1, C_, K)).astype(F32)
    w = rng.standard_normal((1, Hd, S, H, W)).astype(F32)
    # [H, W, C] and [K, C] and [H, W, Hd, S] storage behind the expected shapes, and the unbatched forms; the map as numpy int16
    xt = dev(np.moveaxis(x[0], 0, -1)).permute(2, 0, 1)
    bt = dev(b[0].T).t()
    wt = dev(np.moveaxis(w[0], (0, 1), (-2, -1))).permute(2, 3, 0, 1)
    assert not xt.is_contiguous() and not bt.is_contiguous() and not wt.is_contiguous()
    s = pixel_dot(xt, bt, labels[0], nl, S, Hd)
    assert tuple(s.shape) == (Hd, S, H, W) and same(s, R.dot(x, b, sl, Hd)[0])
    assert same(pixel_softmax(wt, labels[0], nl), R.softmax(w, sl)[0])
    assert same(pixel_mix(bt, wt, labels[0], nl), R.mix(b, w, sl)[0])
    z = pixel_scatter(xt, wt, labels[0], nl, K)
    assert tuple(z.shape) == (C_, K) and torch.equal(z.view(torch.int32), pixel_scatter(dev(x), dev(w), dev(labels), nl, K)[0].view(torch.int32))
    y, alpha = pixel_attention(xt, bt, bt, labels[0], nl, S, Hd, return_weights=True)
    assert tuple(y.shape) == (C_, H, W) and tuple(alpha.shape) == (Hd, S, H, W)
    assert tuple(pixel_slots(labels[0], nl, S).shape) == (S, H, W)


def test_pixel_attention_is_its_composition():
    rng = np.random.default_rng(12)
    N, H, W, K, S, C_, Cv, Hd = 2, 19, 70, 30, 9, 8, 4, 2
    nl, offsets, indices = lists_of([random_pairs(rng, K, 6), path(K)], K)
    labels = random_map(rng, N, H, W, K, "int32", blocks=True)
    lab = dev(labels)
    q, k = rng.standard_normal((N, C_, H, W)).astype(F32), rng.standard_normal((N, C_, K)).astype(F32)
    v, g = rng.standard_normal((N, Cv, K)).astype(F32), rng.standard_normal((N, Cv, H, W)).astype(F32)
    for scale in (None, 0.3):
        leaves = [[dev(t).requires_grad_() for t in (q, k, v)] for _ in range(2)]
        y, alpha = pixel_attention(*leaves[0], lab, nl, S, Hd, scale, return_weights=True)
        y.backward(dev(g))
        factor = torch.tensor(float((C_ // Hd) ** -0.5 if scale is None else scale), dtype=torch.float32).item()
        alpha2 = pixel_softmax(pixel_dot(leaves[1][0] * factor, leaves[1][1], lab, nl, S, Hd), lab, nl)
        y2 = pixel_mix(leaves[1][2], alpha2, lab, nl)
        y2.backward(dev(g))
        assert torch.equal(y.view(torch.int32), y2.view(torch.int32)) and torch.equal(alpha.view(torch.int32), alpha2.view(torch.int32))
        assert torch.equal(pixel_attention(*leaves[0], lab, nl, S, Hd, scale).view(torch.int32), y.view(torch.int32))
        for t, u in zip(*leaves):
            assert torch.equal(t.grad.view(torch.int32), u.grad.view(torch.int32)) and t.grad.abs().max() > 0
        # and the model of the composition
        sl = R.slots(labels, offsets, indices, N, K, S)
        want = R.softmax(R.dot(q * F32(factor), k, sl, Hd), sl)
        assert same(alpha, want) and same(y, R.mix(v, want, sl))


def test_a_side_stream_and_no_host_synchronisation():
    """Every function and every backward on a stream of the caller's and with torch refusing every host synchronisation: the bits of
    the plain call."""
    rng = np.random.default_rng(9)
    N, H, W, K, S, C_, Hd = 2, 33, 129, 40, 9, 4, 2
    g = make_graph([random_pairs(rng, K, 6), random_pairs(rng, K, 4)], K, DEV)
    nl = neighbour_lists(g)
    lab = dev(random_map(rng, N, H, W, K, "int16", blocks=True))
    x, b = dev(rng.standard_normal((N, C_, H, W)).astype(F32)), dev(rng.standard_normal((N, C_, K)).astype(F32))
    gy = dev(rng.standard_normal((N, C_, H, W)).astype(F32))

    def calls():
        xt, bt = x.clone().requires_grad_(), b.clone().requires_grad_()
        y, alpha = pixel_attention(xt, bt, bt, lab, nl, S, Hd, return_weights=True)
        z = pixel_scatter(xt, alpha, lab, g, K)
        (y * gy).sum().backward(retain_graph=True)
        z.sum().backward()
        return y.detach(), alpha.detach(), z.detach(), xt.grad, bt.grad

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
        stream.synchronize()                                                   # this stream only
    for other in (got, side):
        assert other is None or all(np.array_equal(p.cpu().numpy().view(np.uint8), q.cpu().numpy().view(np.uint8)) for p, q in zip(want, other))


def test_the_peak_memory_of_a_scatter_is_its_output_and_its_accumulator():
    """No [N, C, S, H, W] intermediate: the peak rises by the output, the workspace the library asks for and allocator rounding."""
    rng = np.random.default_rng(13)
    N, H, W, K, S, C_, Hd = 2, 64, 128, 50, 9, 8, 2
    nl, _, _ = lists_of([random_pairs(rng, K, 6), random_pairs(rng, K, 6)], K)
    lab = dev(random_map(rng, N, H, W, K, "int16", blocks=True))
    x, w = dev(rng.standard_normal((N, C_, H, W)).astype(F32)), dev(rng.standard_normal((N, Hd, S, H, W)).astype(F32))
    size = C.c_size_t()
    assert B.load_library().fslic_hip_pixel_scatter_workspace_size(N, C_, K, C.byref(size)) == B.FSLIC_OK
    pixel_scatter(x, w, lab, nl, K)                                            # the library is loaded and the module's kernels are resident
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    before = torch.cuda.memory_allocated(DEV)
    z = pixel_scatter(x, w, lab, nl, K)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(DEV) - before
    print("peak rise %d bytes: output %d, workspace %d; [N, C, S, H, W] would be %d" % (rise, z.numel() * 4, size.value, N * C_ * S * H * W * 4))
    assert 0 < rise <= z.numel() * 4 + size.value + 4096
    assert size.value + z.numel() * 4 + 4096 < N * C_ * S * H * W * 4
