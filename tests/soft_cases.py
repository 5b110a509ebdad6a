"""What the GPU tests of soft superpixel assignment share (test_gpu_soft.py, test_gpu_soft_edges.py): the measured bound against the
float64 model of soft_ref.py, the comparison on bits, and one shape's random inputs with the model's results.  No test lives here."""
import torch

import soft_ref as R
from fast_slic_amd.soft import soft_assign, soft_pool, soft_unpool

DEV = torch.device("cuda", 0)
FLOOR = 2.0 ** -20


def rel(x, ref):
    """max |x - ref| / max |ref| (the plain max |x - ref| where the reference is zero everywhere: K = 1 has no gradient to assign)"""
    scale = float(ref.abs().max())
    return float((x.detach().cpu().double() - ref).abs().max()) / (scale if scale > 0 else 1.0)


def hold(name, got, ref64, ref32):
    err, b = rel(got, ref64), rel(ref32, ref64)
    bound = max(8.0 * b, FLOOR)
    print("%-16s err %.3e  b %.3e  bound %.3e  err/bound %.3f" % (name, err, b, bound, err / bound))
    assert err <= bound, "%s: err %.3e above max(8 b, 2^-20) = %.3e" % (name, err, bound)
    return err / bound


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_stages(t, grid, assign, pool, unpool):
    """the three stages and their backwards through one implementation, on the tensors t (F, S, Q, V, gQ, gS, gW, gO) -> dict of
    detached results"""
    leaf = lambda x: x.clone().requires_grad_(True)
    out = {}
    F, S = leaf(t["F"]), leaf(t["S"])
    q = assign(F, S, grid)
    out["assign Q"] = q
    out["assign gF"], out["assign gS"] = torch.autograd.grad((q * t["gQ"]).sum(), (F, S))
    F, Q = leaf(t["F"]), leaf(t["Q"])
    sums, weights = pool(F, Q, grid)
    out["pool sums"], out["pool weights"] = sums, weights
    out["pool gF"], out["pool gQ"] = torch.autograd.grad((sums * t["gS"]).sum() + (weights * t["gW"]).sum(), (F, Q))
    V, Q = leaf(t["V"]), leaf(t["Q"])
    o = unpool(V, Q, grid)
    out["unpool out"] = o
    out["unpool gV"], out["unpool gQ"] = torch.autograd.grad((o * t["gO"]).sum(), (V, Q))
    return {k: v.detach() for k, v in out.items()}


def gpu_pool(f, q, grid):
    return soft_pool(f, q, grid, normalize=False, return_weights=True)


def gpu_stages(t, grid):
    return run_stages(t, grid, soft_assign, gpu_pool, soft_unpool)


def model_stages(t, grid):
    return run_stages(t, grid, R.soft_assign, R.soft_pool_raw, R.soft_unpool)


class Case(object):
    """Random inputs of one shape and the model's results in float64 and float32, computed once.  `adjust` (optional) edits the drawn
    tensors before the model's Q and results are taken from them."""
    NAMES = ("F", "S", "Q", "V", "gQ", "gS", "gW", "gO")

    def __init__(self, H, W, grid, Cc, n=3, adjust=None):
        g = torch.Generator().manual_seed(1000 * H + 10 * W + Cc)
        K = grid[0] * grid[1]
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
        self.H, self.W, self.grid, self.Cc, self.K, self.n = H, W, grid, Cc, K, n
        self.F = rnd(n, Cc, H, W) * 0.5
        first = R.soft_pool(self.F.double(), R.one_hot(n, H, W), grid)
        self.S = (first + rnd(n, Cc, K).double() * (0.6 / Cc ** 0.5)).float()       # spreads Q over the slots
        self.V = rnd(n, Cc, K)
        self.gQ, self.gS, self.gW, self.gO = rnd(n, 9, H, W), rnd(n, Cc, K), rnd(n, K), rnd(n, Cc, H, W)
        if adjust is not None:
            adjust(self)
        self.Q = R.soft_assign(self.F, self.S, grid)                                # the float32 model's Q feeds pool and unpool
        self.ref = {dt: self.run(self.tensors("cpu", dt), R.soft_assign, R.soft_pool_raw, R.soft_unpool)
                    for dt in (torch.float64, torch.float32)}

    def tensors(self, device, dtype=torch.float32, frames=slice(None)):
        return {n: getattr(self, n)[frames].to(device=device, dtype=dtype) for n in self.NAMES}

    def run(self, t, assign, pool, unpool):
        return run_stages(t, self.grid, assign, pool, unpool)

    def gpu(self, frames=slice(None), t=None):
        return self.run(self.tensors(DEV, frames=frames) if t is None else t, soft_assign, gpu_pool, soft_unpool)
