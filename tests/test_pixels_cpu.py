"""CPU tests of the pixels over neighbour lists (fast_slic_amd/pixels.py, the fslic_hip_pixel_* entries): the float32 model
(tests/pixels_ref.py) by hand on a 2 x 3 map over a path of three nodes, its forward and backward formulas against torch's float64
autograd of a dense restatement built from pixel_slots (gather / index_add_), and every argument error refused before any device work
-- ValueError in Python, FSLIC_E_INVALID from the C ABI before its first HIP call, with the words and the order of
csrc/pixelapi.cpp.  No kernel is launched here."""
import os
import re

import numpy as np
import pytest
import torch

import pixels_ref as R
from aggregate_ref import gamma
from fast_slic_amd import _binding as B
from fast_slic_amd import pixels
from fast_slic_amd.pixels import pixel_attention, pixel_dot, pixel_mix, pixel_scatter, pixel_slots, pixel_softmax
from fast_slic_amd.propagate import neighbour_lists
from test_aggregate_cpu import make_graph, numpy_lists, path, random_pairs, star
from test_stream_refusals_cpu import BIG, BYTES, DEVICE, NUL, NULL_ARG, P, label_map, rows_of

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def positive_zeros(a):
    a = np.asarray(a)
    return not a.any() and not np.signbit(a).any()


# ---- the model, by hand ----
# 0 - 1 - 2 with the last entry (row 2's only one) made invalid; the map holds a pixel without a label
HAND_OFFSETS, HAND_INDICES = np.array([0, 1, 3, 4]), np.array([1, 0, 2, 3], np.int32)
HAND_LABELS = np.array([[[0, 1, 1], [2, -1, 1]]], np.int16)


def test_model_by_hand_on_a_map_of_2_x_3_over_a_path_of_three():
    sl = R.slots(HAND_LABELS, HAND_OFFSETS, HAND_INDICES, 1, 3, 2)
    # S = 2 cuts node 1's row (0, 2) after its first entry; label 2's entry names node 3 = K; the pixel without a label has no slot
    assert sl.tolist() == [[[[0, 1, 1], [2, -1, 1]], [[1, 0, 0], [-1, -1, 0]]]]
    assert R.slots(HAND_LABELS, HAND_OFFSETS, HAND_INDICES, 1, 3, 3)[0, 2].tolist() == [[-1, 2, 2], [-1, -1, 2]]
    a = np.array([[[[1, 2, 3], [4, 5, 6]]]], F32)
    b = np.array([[[10, 20, 30]]], F32)
    s = R.dot(a, b, sl, 1)
    assert s.dtype == F32 and s.tolist() == [[[[[10, 40, 60], [120, 0, 120]], [[20, 20, 30], [0, 0, 60]]]]]
    w = np.zeros((1, 1, 2, 2, 3), F32)
    w[:, :, 0], w[:, :, 1] = 1, 2
    assert R.mix(b, w, sl).tolist() == [[[[50, 40, 40], [30, 0, 40]]]]
    # node 0: its own pixel and twice the three pixels of label 1; node 1: its three pixels and twice the pixel of label 0; node 2: its pixel
    assert R.scatter_exact(a, w, HAND_LABELS, sl, 3).view(F32).tolist() == [[[23, 13, 4]]]
    assert R.scatter_sum64(a, w, sl, 3)[0].tolist() == [[[23, 13, 4]]] and R.scatter_sum64(-a, w, sl, 3)[1].tolist() == [[[23, 13, 4]]]
    alpha = R.softmax(np.zeros_like(w), sl)
    assert alpha.tolist() == [[[[[0.5, 0.5, 0.5], [1, 0, 0.5]], [[0.5, 0.5, 0.5], [0, 0, 0.5]]]]]
    assert positive_zeros(alpha[0, 0, :, 1, 1]) and positive_zeros(alpha[0, 0, 1, 1, 0]) and positive_zeros(s[0, 0, :, 1, 1])
    # scores ln 3 apart: 3 / 4 and 1 / 4 within an ulp of the exponential
    alpha = R.softmax(np.log(3) * w, sl)
    assert np.allclose(alpha[0, 0, :, 0, 0], [0.25, 0.75], rtol=1e-6) and alpha[0, 0, :, 1, 0].tolist() == [1, 0]
    # the backward: t = sum alpha g, alpha (g - t); a pixel with one slot gets 0 = 1 * (g - g)
    g = np.zeros_like(w)
    g[:, :, 0], g[:, :, 1] = 8, 4
    half = R.softmax(np.zeros_like(w), sl)
    assert R.softmax_backward(half, g, sl).tolist() == [[[[[1, 1, 1], [0, 0, 1]], [[-1, -1, -1], [0, 0, -1]]]]]


def test_the_exact_scatter_refuses_a_partial_that_is_no_float32():
    sl = R.slots(HAND_LABELS, HAND_OFFSETS, HAND_INDICES, 1, 3, 1)
    x = np.array([[[[1, 1, 2.0 ** 30], [1, 1, 1]]]], F32)                      # label 1: 1 + 2^30 + 1 needs 31 bits
    with pytest.raises(ValueError, match="not representable"):
        R.scatter_exact(x, np.ones((1, 1, 1, 2, 3), F32), HAND_LABELS, sl, 3)
    # below 2^-96 a partial is truncated, and a zero total is +0.0
    x = np.array([[[[5 * 2.0 ** -100, 2.0 ** -97, 2.0 ** -97], [-1, 1, -(2.0 ** -96)]]]], F32)
    bits = R.scatter_exact(x, np.ones((1, 1, 1, 2, 3), F32), HAND_LABELS, sl, 3)
    assert bits.tolist() == [[[0, 0, 0xBF800000]]]


# ---- against float64: torch's autograd of a dense restatement built from pixel_slots ----
def at_nodes64(t, sl):
    """t [N, C, K] at the node of every slot -> [N, C, S, H, W], zero where the slot is empty."""
    N = t.shape[0]
    got = t[torch.arange(N).view(N, 1, 1, 1), :, sl.clamp(min=0).long()]           # [N, S, H, W, C]
    return got.permute(0, 4, 1, 2, 3) * (sl >= 0)[:, None]


def dot64(a, b, sl, Hd):
    N, Cc, H, W = a.shape
    return (a[:, :, None] * at_nodes64(b, sl)).reshape(N, Hd, Cc // Hd, sl.shape[1], H, W).sum(2)


def mix64(values, weight, sl):
    D = values.shape[1] // weight.shape[1]
    return (weight.repeat_interleave(D, dim=1) * at_nodes64(values, sl)).sum(2)


def scatter64(x, weight, sl, K):
    N, Cc = x.shape[:2]
    prod = weight.repeat_interleave(Cc // weight.shape[1], dim=1) * x[:, :, None] * (sl >= 0)[:, None]
    node = (torch.arange(N).view(N, 1, 1, 1) * K + sl.clamp(min=0).long()).reshape(-1)
    flat = torch.zeros((Cc, N * K), dtype=x.dtype).index_add(1, node, prod.transpose(0, 1).reshape(Cc, -1))
    return flat.reshape(Cc, N, K).transpose(0, 1)


def softmax64(s, sl):
    masked = torch.where((sl >= 0)[:, None], s, torch.full_like(s, -float("inf")))
    m = masked.detach().amax(2, keepdim=True)
    e = torch.exp(masked - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))         # an empty slot: exp(-inf) = 0
    return e / e.sum(2, keepdim=True).clamp(min=1e-300)


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def case(seed, N, K, degree, H, W, S):
    """Random lists with a hub in the last frame, a random map with labels outside [0, K), and both kinds of slots."""
    rng = np.random.default_rng(seed)
    frames = [random_pairs(rng, K, degree) for _ in range(N - 1)] + [path(K) + star(K, min(10, K - 1))]
    nl = neighbour_lists(make_graph(frames, K))
    labels = rng.integers(-1, K + 1, (N, H, W)).astype(np.int32)
    sl = pixel_slots(torch.from_numpy(labels), nl, S)
    offsets, indices = numpy_lists(nl)
    assert sl.dtype == torch.int32 and np.array_equal(sl.numpy(), R.slots(labels, offsets, indices, N, K, S))
    return rng, nl, labels, sl


CASES = [(0, 1, 5, 2, 3, 4, 1, 1, 1), (1, 2, 12, 4, 5, 7, 4, 6, 2), (2, 3, 30, 6, 4, 9, 9, 8, 4), (3, 1, 40, 3, 6, 5, 32, 3, 1)]      # seed, N, K, degree, H, W, S, C, Hd


@pytest.mark.parametrize("seed,N,K,degree,H,W,S,C,Hd", CASES)
def test_model_against_float64_autograd(seed, N, K, degree, H, W, S, C, Hd):
    """Every forward and every gradient of rule 5, the model's float32 folds against float64: a fold of n terms is within gamma(n) *
    sum |terms| (pixels_ref's docstring); the scatter's model is the float64 sum of float32 products, one rounding a term."""
    rng, nl, labels, sl = case(seed, N, K, degree, H, W, S)
    s_np, D = sl.numpy().astype(np.int64), C // Hd
    a, x = (rng.standard_normal((N, C, H, W)).astype(F32) for _ in range(2))
    b, v = (rng.standard_normal((N, C, K)).astype(F32) for _ in range(2))
    w, gs = (rng.standard_normal((N, Hd, S, H, W)).astype(F32) for _ in range(2))
    gp, gk = rng.standard_normal((N, C, H, W)).astype(F32), rng.standard_normal((N, C, K)).astype(F32)
    slack = 1 + 2.0 ** -10

    def close(got, want, terms, n):
        assert (np.abs(np.asarray(got, np.float64) - want.numpy()) <= gamma(n) * terms.numpy() * slack + 1e-300).all()
        assert np.abs(want.numpy()).max() > 0

    # the dot, and its gradients: a mix and a scatter
    la, lb = t64(a).requires_grad_(), t64(b).requires_grad_()
    out = dot64(la, lb, sl, Hd)
    out.backward(t64(gs))
    close(R.dot(a, b, s_np, Hd), out.detach(), dot64(t64(np.abs(a)), t64(np.abs(b)), sl, Hd), D)
    close(R.mix(b, gs, s_np), la.grad, mix64(t64(np.abs(b)), t64(np.abs(gs)), sl), S)
    got, mag = R.scatter_sum64(a, gs, s_np, K)
    close(got, lb.grad, t64(mag), 1)
    assert np.allclose(mag, scatter64(t64(np.abs(a)), t64(np.abs(gs)), sl, K).numpy(), rtol=1e-6, atol=0)
    # the mix, and its gradients: a scatter and a dot
    lv, lw = t64(v).requires_grad_(), t64(w).requires_grad_()
    out = mix64(lv, lw, sl)
    out.backward(t64(gp))
    close(R.mix(v, w, s_np), out.detach(), mix64(t64(np.abs(v)), t64(np.abs(w)), sl), S)
    got, mag = R.scatter_sum64(gp, w, s_np, K)
    close(got, lv.grad, t64(mag), 1)
    close(R.dot(gp, v, s_np, Hd), lw.grad, dot64(t64(np.abs(gp)), t64(np.abs(v)), sl, Hd), D)
    # the scatter, and its gradients: a mix and a dot
    lx, lw = t64(x).requires_grad_(), t64(w).requires_grad_()
    out = scatter64(lx, lw, sl, K)
    out.backward(t64(gk))
    got, mag = R.scatter_sum64(x, w, s_np, K)
    close(got, out.detach(), t64(mag), 1)
    close(R.mix(gk, w, s_np), lx.grad, mix64(t64(np.abs(gk)), t64(np.abs(w)), sl), S)
    close(R.dot(x, gk, s_np, Hd), lw.grad, dot64(t64(np.abs(x)), t64(np.abs(gk)), sl, Hd), D)
    # the softmax and its backward
    ls = t64(w).requires_grad_()
    alpha64 = softmax64(ls, sl)
    alpha64.backward(t64(gs))
    alpha = R.softmax(w, s_np)
    rel = R.alpha_bound(w, s_np)
    assert (np.abs(alpha - alpha64.detach().numpy()) <= rel * alpha64.detach().numpy()).all()
    assert positive_zeros(alpha[np.broadcast_to((s_np < 0)[:, None], alpha.shape)])
    total = alpha.astype(np.float64).sum(2)
    assert (np.abs(total[np.broadcast_to((s_np[:, :1] >= 0), total.shape)] - 1) < 1e-5).all()
    # the backward from float64's alpha rounded to float32: its error is inside rel
    a32 = alpha64.detach().numpy().astype(F32)
    got = R.softmax_backward(a32, gs, s_np)
    assert (np.abs(got - ls.grad.numpy()) <= R.softmax_backward_bound(alpha64.detach().numpy(), gs, rel, s_np) + 1e-300).all()
    assert positive_zeros(got[np.broadcast_to((s_np < 0)[:, None], got.shape)]) and (S == 1 or np.abs(ls.grad.numpy()).max() > 0)


def test_slots_of_every_kind_of_lists():
    nl = neighbour_lists(make_graph([path(5), star(5, 3)], 5))
    lab = torch.tensor([[[0, 2, 4], [5, -1, 3]], [[2, 2, 0], [1, 4, 9]]], dtype=torch.int64)
    want = R.slots(lab.numpy(), *numpy_lists(nl), 2, 5, 4)
    for lists, kw in ((nl, {}), (make_graph([path(5), star(5, 3)], 5), {}), ((nl.offsets, nl.indices), dict(num_components=5))):
        for labels in (lab, lab.to(torch.int32), lab.to(torch.int16), lab.numpy().astype(np.int16)):
            assert np.array_equal(pixel_slots(labels, lists, 4, **kw).numpy(), want)
    assert np.array_equal(pixel_slots(lab[1], neighbour_lists(make_graph([star(5, 3)], 5)), 4).numpy(), want[1])      # [H, W] -> [S, H, W]
    # garbage offsets are clamped, an end before its start is an empty row, and without entries only slot 0 is left
    offsets = torch.tensor([7, -3, 100, 2, 1, 0, 5, 5, 9, 9, 10], dtype=torch.int64)
    indices = torch.tensor([4, -1, 5, 0, 3], dtype=torch.int32)
    got = pixel_slots(lab, (offsets, indices), 6, num_components=5)
    assert np.array_equal(got.numpy(), R.slots(lab.numpy(), offsets.numpy(), indices.numpy(), 2, 5, 6))
    got = pixel_slots(lab, (torch.zeros(11, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)), 3, num_components=5)
    assert (got[:, 1:] == -1).all() and np.array_equal(got[:, 0].numpy(), np.where((lab >= 0) & (lab < 5), lab, -1))


# ---- argument errors: all before any device work (a CPU tensor is the last thing refused) ----
G = make_graph([path(5), star(5, 3)], 5)                                   # N = 2, K = 5
NL = neighbour_lists(G)
PAIR = (NL.offsets, NL.indices)
A = torch.zeros((2, 4, 3, 6))
BK = torch.zeros((2, 4, 5))
LAB = torch.zeros((2, 3, 6), dtype=torch.int32)
WT = torch.zeros((2, 2, 3, 3, 6))                                          # Hd = 2, S = 3


def refused(match, fn, *args, **kw):
    with pytest.raises(ValueError, match=match):
        fn(*args, **kw)


def test_bad_dot_arguments():
    for lists in (G, NL, PAIR):
        refused("a must be float32", pixel_dot, A.double(), BK, LAB, lists, 3)
        refused(r"a must be \[C, H, W\] or \[N, C, H, W\]", pixel_dot, torch.zeros((3, 6)), BK, LAB, lists, 3)
        refused("a must be a torch tensor", pixel_dot, None, BK, LAB, lists, 3)
        refused("a must not be empty", pixel_dot, torch.zeros((2, 0, 3, 6)), BK, LAB, lists, 3)
        refused(r"b must be \[N, C, K\] with N = 2", pixel_dot, A, BK[0], LAB, lists, 3)
        refused(r"b must be \[N, C, K\] with N = 2", pixel_dot, A, torch.zeros((3, 4, 5)), LAB, lists, 3)
        refused(r"b must be \[C, K\]", pixel_dot, A[0], BK, LAB[0], lists, 3)
        refused("b must have 4 channels", pixel_dot, A, torch.zeros((2, 3, 5)), LAB, lists, 3)
        refused("K, the last dimension of b, must be in", pixel_dot, A, torch.zeros((2, 4, 65535)), LAB, lists, 3)
        refused("labels must be int16", pixel_dot, A, BK, LAB.to(torch.uint8), lists, 3)
        refused("labels must be int16", pixel_dot, A, BK, LAB.numpy().astype(np.float32), lists, 3)
        refused(r"labels must have shape \(2, 3, 6\)", pixel_dot, A, BK, LAB[0], lists, 3)
        refused(r"labels must have shape \(3, 6\)", pixel_dot, A[0], BK[0], LAB, lists, 3)
        refused("labels must be a numpy array or a torch tensor", pixel_dot, A, BK, None, lists, 3)
        refused(r"the values have 2 of 6|graph offsets must be \[N \* K \+ 1\] = \[13\]", pixel_dot, A, torch.zeros((2, 4, 6)), LAB, lists, 3)
        for slots in (0, 33, 2.0, True, None, "9"):
            refused(r"slots must be an integer in \[1, 32\]", pixel_dot, A, BK, LAB, lists, slots)
        for heads in (0, -1, 1.0, True):
            refused("heads must be a positive integer", pixel_dot, A, BK, LAB, lists, 3, heads)
        refused("C = 4 is not a multiple of heads = 3", pixel_dot, A, BK, LAB, lists, 3, 3)
    refused("a pair", pixel_dot, A, BK, LAB, None, 3)
    refused("graph indices must be int32", pixel_dot, A, BK, LAB, (NL.offsets, NL.indices.long()), 3)


def test_bad_softmax_mix_and_scatter_arguments():
    for lists, kw in ((G, {}), (NL, {}), (PAIR, dict(num_components=5))):
        refused(r"scores must be \[Hd, S, H, W\] or \[N, Hd, S, H, W\]", pixel_softmax, torch.zeros((2, 3, 6)), LAB, lists, **kw)
        refused("scores must be float32", pixel_softmax, WT.double(), LAB, lists, **kw)
        refused("scores must not be empty", pixel_softmax, torch.zeros((2, 0, 3, 3, 6)), LAB, lists, **kw)
        refused(r"slots must be an integer in \[1, 32\], got 33", pixel_softmax, torch.zeros((2, 1, 33, 3, 6)), LAB, lists, **kw)
        refused(r"labels must have shape \(2, 3, 6\)", pixel_softmax, WT, LAB[:, :, :5], lists, **kw)
        refused(r"weight must be \[Hd, S, H, W\] or \[N, Hd, S, H, W\]", pixel_mix, BK, torch.zeros((3, 6)), LAB, lists)
        refused(r"values must be \[N, C, K\] with N = 2", pixel_mix, BK[0], WT, LAB, lists)
        refused("Cv = 3 is not a multiple of heads = 2", pixel_mix, torch.zeros((2, 3, 5)), WT, LAB, lists)
        refused(r"weight must be \[N, Hd, S, H, W\]", pixel_scatter, A, WT[0], LAB, lists, 5)
        refused("weight must be one value per head, slot and pixel of the 2 frames of 3 x 6", pixel_scatter, A, torch.zeros((2, 2, 3, 3, 5)), LAB, lists, 5)
        refused("x must be float32", pixel_scatter, A.half(), WT, LAB, lists, 5)
        refused("C = 4 is not a multiple of heads = 3", pixel_scatter, A, torch.zeros((2, 3, 3, 3, 6)), LAB, lists, 5)
        for K in (0, 65535, 5.0, None, True):
            refused("num_components must be", pixel_scatter, A, WT, LAB, lists, K)
        refused(r"the values have 2 of 6|graph offsets must be \[N \* K \+ 1\] = \[13\]", pixel_scatter, A, WT, LAB, lists, 6)
    refused("a raw pair .offsets, indices. needs num_components", pixel_softmax, WT, LAB, PAIR)
    refused("a raw pair .offsets, indices. needs num_components", pixel_slots, LAB, PAIR, 3)
    refused("num_components must be an integer", pixel_softmax, WT, LAB, PAIR, num_components=5.0)
    refused("the node tensors have K = 5 nodes, num_components is 6", pixels._graph_size, NL, 2, 6, 5)
    refused(r"slots must be an integer in \[1, 32\]", pixel_slots, LAB, NL, 0)
    refused(r"labels must be \[H, W\] or \[N, H, W\]", pixel_slots, LAB[0, 0], NL, 3)


def test_bad_attention_arguments():
    V = torch.zeros((2, 6, 5))
    refused("key must have 4 channels", pixel_attention, A, torch.zeros((2, 2, 5)), V, LAB, NL, 3)
    refused("values must have K = 5 nodes", pixel_attention, A, BK, torch.zeros((2, 6, 4)), LAB, NL, 3)
    refused(r"values must be \[N, C, K\] with N = 2", pixel_attention, A, BK, V[0], LAB, NL, 3)
    refused("Cv = 6 is not a multiple of heads = 4", pixel_attention, A, BK, V, LAB, NL, 3, 4)
    for scale in (float("nan"), float("inf"), "1", True):
        refused("scale must be None or a finite number", pixel_attention, A, BK, V, LAB, NL, 3, 2, scale)
    refused("query must be on a ROCm GPU", pixel_attention, A, BK, V, LAB, NL, 3, 2, 0.5, True)


def test_2_to_the_31_limits():
    """Tensors of the sizes in question without their memory: one element expanded."""
    text = r"N \* C \* H \* W, N \* heads \* slots \* H \* W, N \* C \* K and the number of neighbour entries must be below 2\^31"
    one, lab = torch.zeros(1), torch.zeros(1, dtype=torch.int32)
    nl = (torch.zeros(1, dtype=torch.int64).expand(5 + 1), torch.zeros(4, dtype=torch.int32))
    b = torch.zeros((1, 2, 5))
    for H, W, ok in ((1 << 15, 1 << 15, False), (1 << 15, (1 << 15) - 1, True)):       # N * C * H * W with C = 2
        a = one.expand(1, 2, H, W)
        refused("no CPU fallback" if ok else text, pixel_dot, a, b, lab.expand(1, H, W), nl, 1)
    a = one.expand(1, 2, 1 << 13, 1 << 13)                                             # N * heads * slots * H * W: 2 * 16 * 2^26
    refused(text, pixel_dot, a, b, lab.expand(1, 1 << 13, 1 << 13), nl, 16, 2)
    refused("no CPU fallback", pixel_dot, a, b, lab.expand(1, 1 << 13, 1 << 13), nl, 15, 2)
    refused(text, pixel_softmax, one.expand(1, 2, 16, 1 << 13, 1 << 13), lab.expand(1, 1 << 13, 1 << 13), nl, num_components=5)
    K = 1 << 15                                                                        # N * C * K
    nk = (torch.zeros(1, dtype=torch.int64).expand(K + 1), torch.zeros(4, dtype=torch.int32))
    refused(text, pixel_mix, one.expand(1, 1 << 16, K), one.expand(1, 1, 1, 1, 1), lab.expand(1, 1, 1), nk)
    refused("no CPU fallback", pixel_mix, one.expand(1, (1 << 16) - 1, K), one.expand(1, 1, 1, 1, 1), lab.expand(1, 1, 1), nk)
    many = (nl[0], torch.zeros(1, dtype=torch.int32).expand(1 << 31))                  # nnz
    refused(text, pixel_scatter, one.expand(1, 2, 1, 1), one.expand(1, 1, 1, 1, 1), lab.expand(1, 1, 1), many, 5)
    many = (nl[0], torch.zeros(1, dtype=torch.int32).expand((1 << 31) - 1))
    refused("no CPU fallback", pixel_scatter, one.expand(1, 2, 1, 1), one.expand(1, 1, 1, 1, 1), lab.expand(1, 1, 1), many, 5)


def test_cpu_tensors_are_refused_after_every_other_check():
    for lists, kw in ((G, {}), (NL, {}), (PAIR, dict(num_components=5))):
        refused("a must be on a ROCm GPU, got device cpu .there is no CPU fallback.", pixel_dot, A, BK, LAB, lists, 3, 2)
        refused("scores must be on a ROCm GPU", pixel_softmax, WT, LAB, lists, **kw)
        refused("values must be on a ROCm GPU", pixel_mix, BK, WT, LAB, lists)
        refused("x must be on a ROCm GPU", pixel_scatter, A, WT, LAB.numpy().astype(np.int16), lists, 5)
    refused("a must be on a ROCm GPU", pixel_dot, A[0], BK[0], LAB[0], neighbour_lists(make_graph([path(5)], 5)), 3)      # unbatched


def test_the_tensors_are_handed_to_one_device_in_this_order(monkeypatch):
    """No GPU here, let alone two: _tensors.one_device refuses two GPUs first and a CPU tensor last (tests/test_aggregate_cpu.py).  A
    label map that is not on a GPU names none: it is uploaded."""
    seen = []

    def one_device(tensors):
        seen.append([name for _, name in tensors])
        raise ValueError("stop")

    monkeypatch.setattr(pixels.T, "one_device", one_device)
    refused("stop", pixel_dot, A, BK, LAB, NL, 3)
    refused("stop", pixel_softmax, WT, LAB, G)
    refused("stop", pixel_mix, BK, WT, LAB, PAIR)
    refused("stop", pixel_scatter, A, WT, LAB, NL, 5)
    refused("stop", pixel_attention, A, BK, BK, LAB, NL, 3)
    assert seen == [["a", "b", "nl.offsets", "nl.indices"], ["scores", "graph.edge_index", "graph.offsets"],
                    ["values", "weight", "graph offsets", "graph indices"], ["x", "weight", "nl.offsets", "nl.indices"],
                    ["query", "key", "values", "nl.offsets", "nl.indices"]]


def test_the_package_itself_does_not_import_the_module():
    assert re.search(r"\bpixels\b", open(os.path.join(ROOT, "fast_slic_amd", "__init__.py")).read()) is None
    assert pixels.__all__ == ["pixel_dot", "pixel_softmax", "pixel_mix", "pixel_scatter", "pixel_attention", "pixel_slots"]
    assert "bit for bit" in pixels.__doc__ and "4 N Hd S H W bytes" in pixels.__doc__


# ---- the C ABI: FSLIC_E_INVALID before any HIP call (a bogus non-NULL pointer is never touched) ----
NAMES = ["fslic_hip_pixel_dot", "fslic_hip_pixel_mix", "fslic_hip_pixel_softmax", "fslic_hip_pixel_scatter_workspace_size", "fslic_hip_pixel_scatter"]


def lib():
    return B.load_library()


def test_exports():
    header = open(os.path.join(ROOT, "include", "fslic_hip.h")).read()
    assert [n for n in B.EXPORTS if "_pixel_" in n] == NAMES and all(hasattr(lib(), n) and "int %s(" % n in header for n in NAMES)
    assert B.EXPORTS.index("fslic_hip_message_reduce") < B.EXPORTS.index(NAMES[0])         # behind the message entries
    assert B.EXPORTS.index(NAMES[-1]) + 1 == B.EXPORTS.index("fslic_hip_pool_workspace_size")      # in front of the pinned tail of the table


# streamapi.h's checks of a [N][C][K] array and of a label map, then pixelapi.cpp's own in source order.  (N = 0 leaves no way to the
# products; H = 0 none to the pixel counts.)
CELLS = [("stream", dict(device=-1), b"device must be >= 0"), ("stream", dict(N=0), b"N must be positive"), ("stream", dict(C=0), b"C must be positive"),
         ("stream", dict(K=65535), b"K must be in [1, 65534]"), ("stream", dict(N=1 << 16, K=1 << 15), b"N * C * K must be below 2^31")]
MAP = [("stream", args, text) for _, args, text in label_map()]
OWN = [("pixel:1", dict(S=0), b"S must be in [1, 32]"), ("pixel:2", dict(heads=0), b"heads must be positive"),
       ("pixel:3", dict(heads=3), b"C must be a multiple of heads"),
       ("pixel:4", dict(N=8, H=1 << 14, W=1 << 13), b"N * C * H * W must be below 2^31"),
       ("pixel:5", dict(N=1, S=32, H=1 << 13, W=1 << 13), b"N * heads * S * H * W must be below 2^31"),
       ("stream", dict(nnz=-1), b"nnz must be in [0, 2^31)")]
CALL = dict(device=DEVICE, stream=NUL, N=2, C=4, H=3, W=6, K=5, S=3, heads=2, nnz=14, label_type=1, labels=P, offsets=P, indices=P)
LISTS = ["labels", "offsets", "indices"]

# (entry, valid arguments, checks in source order, the pointers refused alone)
TABLE = [
    ("fslic_hip_pixel_dot", dict(CALL, a=P, b=P, out=P),
     CELLS + MAP + OWN + [("pixel:6", dict(labels=NUL, a=NUL, out=NUL), NULL_ARG)], LISTS + ["a", "b", "out"]),
    ("fslic_hip_pixel_mix", dict(CALL, values=P, weight=P, out=P),
     CELLS + MAP + OWN + [("pixel:7", dict(offsets=NUL, weight=NUL), NULL_ARG)], LISTS + ["values", "weight", "out"]),
    ("fslic_hip_pixel_softmax", dict(CALL, backward=1, scores=P, grad=P, out=P),
     CELLS + MAP + OWN + [("pixel:8", dict(backward=2), b"backward must be 0 or 1"), ("pixel:9", dict(indices=NUL, grad=NUL), NULL_ARG)],
     LISTS + ["scores", "grad", "out"]),
    ("fslic_hip_pixel_scatter", dict(CALL, x=P, weight=P, out=P, workspace=P, workspace_bytes=BIG),
     CELLS + MAP + OWN + [("pixel:10", dict(x=NUL, workspace=NUL), NULL_ARG),
                          ("stream", dict(workspace_bytes=2 * 4 * 5 * 56 - 1), b"workspace too small: 2240 bytes needed")],
     LISTS + ["x", "weight", "out", "workspace"]),
]
REFUSALS = [pytest.param(name, args, text, id="%s-%d-%s" % (name[len("fslic_hip_"):], i, site))
            for name, valid, checks, _ in TABLE for i, (site, args, text) in enumerate(rows_of(valid, checks))]
ALONE = [pytest.param(name, dict(valid, **{p: NUL}), id="%s-%s" % (name[len("fslic_hip_"):], p)) for name, valid, _, ps in TABLE for p in ps]


def test_the_table_holds_every_entry_and_reaches_every_site():
    assert [name for name, _, _, _ in TABLE] == [n for n in NAMES if not n.endswith("_size")]
    for name, valid, _, _ in TABLE:
        assert len(valid) == len(dict((n, a) for n, _, a in B.SIGNATURES)[name]), name
    source = open(os.path.join(ROOT, "fast_slic_amd", "csrc", "pixelapi.cpp")).read()
    sites = source.count("fail(FSLIC_E_INVALID")
    reached = {site for _, _, checks, _ in TABLE for site, _, _ in checks if site != "stream"}
    assert sites == 10 and reached == {"pixel:%d" % (i + 1) for i in range(sites)}


@pytest.mark.parametrize("name,args,text", REFUSALS)
def test_refused_with_these_words(name, args, text):
    assert (getattr(lib(), name)(*args.values()), lib().fslic_hip_last_error()) == (B.FSLIC_E_INVALID, text)


@pytest.mark.parametrize("name,args", ALONE)
def test_every_pointer_is_refused_alone(name, args):
    assert (getattr(lib(), name)(*args.values()), lib().fslic_hip_last_error()) == (B.FSLIC_E_INVALID, NULL_ARG)


def test_without_entries_the_indices_and_a_forward_softmax_the_gradient_may_be_null():
    """The next refusal is then the next pointer's: no HIP call is reached with a NULL that is read."""
    for name, valid, _, ps in TABLE:
        args = dict(valid, nnz=0, indices=NUL, out=NUL)
        assert (getattr(lib(), name)(*args.values()), lib().fslic_hip_last_error()) == (B.FSLIC_E_INVALID, NULL_ARG), name
    args = dict(TABLE[2][1], backward=0, grad=NUL, out=NUL)
    assert (lib().fslic_hip_pixel_softmax(*args.values()), lib().fslic_hip_last_error()) == (B.FSLIC_E_INVALID, NULL_ARG)


def test_the_scatter_workspace_is_the_accumulator():
    import ctypes as C
    size = C.c_size_t()
    assert lib().fslic_hip_pixel_scatter_workspace_size(2, 4, 5, C.byref(size)) == B.FSLIC_OK and size.value == 2 * 4 * 5 * 7 * 8
    assert (lib().fslic_hip_pixel_scatter_workspace_size(2, 4, 5, None), lib().fslic_hip_last_error()) == (B.FSLIC_E_INVALID, NULL_ARG)
    for args, text in (((0, 4, 5), b"N must be positive"), ((2, 0, 5), b"C must be positive"), ((2, 4, 0), b"K must be in [1, 65534]"),
                       ((1 << 16, 1, 1 << 15), b"N * C * K must be below 2^31")):
        assert (lib().fslic_hip_pixel_scatter_workspace_size(*args, BYTES), lib().fslic_hip_last_error()) == (B.FSLIC_E_INVALID, text)
