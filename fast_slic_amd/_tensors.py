"""What the torch-tensor modules share (pool, rag, compare, crf_torch, soft, connect, merge, regions, frames): the library with an entry
present, the helpers of a call, the constants of the C ABI, the argument checks and the choice of the GPU.  A new tensor module takes
these from here and keeps only the checks whose text is its own.  This module imports torch; the package itself does not import it.
"""
import ctypes as C
import numbers

import numpy as np
import torch

from . import _binding as B

LABEL_TYPE = {torch.int16: 0, torch.int32: 1, torch.int64: 2}              # FSLIC_LABEL_*: int16 is read as uint16 (-1 = 0xFFFF)
NUMPY_LABELS = (np.int16, np.uint16, np.int32, np.int64)
MEMBER_TYPE = {torch.int32: 1, torch.int64: 2}                             # FSLIC_LABEL_I32, FSLIC_LABEL_I64
MAX_COMPONENTS = 65534


def library(symbol, what):
    """The loaded library, which must have `symbol`; `what` names its feature, e.g. library("fslic_hip_pool", "pooling entry points")."""
    lib = B.load_library()
    if not hasattr(lib, symbol):
        raise RuntimeError("fast_slic_amd: the loaded library has no %s; rebuild it" % what)
    return lib


# ---- the helpers of a call ----
def stream(dev):
    """The stream argument of an entry: torch's current stream of `dev`."""
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def ptr(t, cond=True):
    """The device pointer of `t`; None (NULL) without a tensor or where `cond` does not hold."""
    return t.data_ptr() if t is not None and cond else None


def scratch(dev, size_entry, *sizes):
    """Scratch memory from torch's caching allocator, as many bytes as the library's `size_entry` asks for `sizes` -> (tensor, bytes)."""
    nbytes = C.c_size_t()
    B._check(size_entry(*sizes, C.byref(nbytes)))
    return torch.empty(nbytes.value, dtype=torch.uint8, device=dev), nbytes.value


def batch_of(t, batched):
    """`t` as a contiguous [N, ...] tensor: an unbatched one becomes [1, ...]."""
    return (t if batched else t.unsqueeze(0)).contiguous()


def labels_on(labels, device, batched=True):
    """Contiguous device tensor of the labels, [1, H, W] for an unbatched map, and its FSLIC_LABEL_* code."""
    if isinstance(labels, np.ndarray):
        a = np.ascontiguousarray(labels)
        if a.dtype == np.uint16:
            a = a.view(np.int16)
        labels = torch.from_numpy(a)
    lab = labels.to(device=device).contiguous()
    return lab if batched else lab.unsqueeze(0), LABEL_TYPE[lab.dtype]


# ---- argument checks: all of them run before any device work ----
def check_tensor(t, what, dtypes, shape_text, ok_shape):
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a torch tensor" % what)
    if t.dtype not in dtypes:
        raise ValueError("%s must be %s, got %s" % (what, " or ".join(str(d).replace("torch.", "") for d in dtypes), t.dtype))
    if not ok_shape(tuple(t.shape)):
        raise ValueError("%s must be %s, got shape %s" % (what, shape_text, tuple(t.shape)))


def check_float_map(t, ranks, what, shape_text):
    """A float32 tensor of one of `ranks` that is not empty.  It is on the path of every pooling call, so the plain tests come first
    and check_tensor only words the refusal."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() not in ranks:
        check_tensor(t, what, (torch.float32,), shape_text, lambda s: False)
    if t.numel() == 0:
        raise ValueError("%s must not be empty, got shape %s" % (what, tuple(t.shape)))


def check_label_map(t, what):
    if not isinstance(t, (np.ndarray, torch.Tensor)):
        raise ValueError("%s must be a numpy array or a torch tensor" % what)
    if t.ndim not in (2, 3):
        raise ValueError("%s must be [H, W] or [N, H, W], got shape %s" % (what, tuple(t.shape)))
    if 0 in t.shape:
        raise ValueError("%s must not be empty, got shape %s" % (what, tuple(t.shape)))
    ok = t.dtype.type in NUMPY_LABELS if isinstance(t, np.ndarray) else t.dtype in LABEL_TYPE
    if not ok:
        raise ValueError("%s must be int16 (Slic.iterate's map), int32 or int64, got %s" % (what, t.dtype))


def check_count(K, what):
    """-> K, an integer in [1, 65534]: num_components, num_other."""
    if isinstance(K, bool) or not isinstance(K, numbers.Integral):
        raise ValueError("%s must be an integer" % what)
    K = int(K)
    if not 1 <= K <= MAX_COMPONENTS:
        raise ValueError("%s must be in [1, %d], got %d" % (what, MAX_COMPONENTS, K))
    return K


def check_device(t, what):
    if t.device.type != "cuda":
        raise ValueError("%s must be on a ROCm GPU, got device %s (there is no CPU fallback)" % (what, t.device))


NO_DEVICE_PARAMETER = object()


def one_device(tensors, device=NO_DEVICE_PARAMETER):
    """The single GPU that `tensors` ((tensor, numpy array or None, name), ...) name, and `device` where the caller has such a
    parameter (None: nothing asked for).  Torch tensors must already be there, and on the same one; numpy arrays are the caller's to
    upload.  Two GPUs are refused first and a CPU tensor is the last thing refused.  With a `device` parameter and nothing that names
    a GPU the answer is torch's current one."""
    asked = device is not NO_DEVICE_PARAMETER
    given = [(t, what, t.device) for t, what in tensors if t is not None and not isinstance(t, np.ndarray)]
    devs = {d for _, _, d in given if d.type == "cuda"}
    device = torch.device(device) if asked and device is not None else None
    if device is not None and device.type == "cuda" and device.index is not None:
        devs.add(device)
    if len(devs) > 1:
        names, rule = (tensors, "and device must name one GPU") if asked else (given, "must be on one GPU")
        raise ValueError("%s %s, got %s" % (", ".join(n[1] for n in names), rule, sorted(str(d) for d in devs)))
    for t, what, d in given:
        if d not in devs:
            check_device(t, what)
    if device is not None and device.type != "cuda":
        raise ValueError("device must be a ROCm GPU, got %s (there is no CPU fallback)" % device)
    return devs.pop() if devs else torch.device("cuda", torch.cuda.current_device())
