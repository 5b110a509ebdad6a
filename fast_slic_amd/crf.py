"""SimpleCRF / SimpleCRFFrame: the surface of the reference's fast_slic.crf (csimple_crf.pyx) over the C ABI of include/fslic_hip.h.

Mean-field inference of a Potts CRF over the superpixel graph, spatial edges inside each frame and temporal edges between consecutive
frames.  Frames are filled on the host (no GPU needed for that); `inference()` runs on the GPU (crf.hip) and is bit-identical to the
reference's.  Deliberate differences from the pyx are listed in include/fslic_hip.h next to the entry points; here they surface as
ValueError where the reference has undefined behaviour (out-of-range neighbours, classes or nodes, inference without frames).
"""
import ctypes as C

import numpy as np

from . import _binding as B

__all__ = ["SimpleCRF", "SimpleCRFFrame"]

_PARAMS = ("spatial_w", "temporal_w", "spatial_srgb", "temporal_srgb", "spatial_sxy", "spatial_smooth_w", "spatial_smooth_sxy")


class _Params(C.Structure):
    _fields_ = [(n, C.c_float) for n in _PARAMS]          # SimpleCRFParams, src/simple-crf.h:11-19


def _lib():
    return B.load_library()


def _f32_2d(a, shape, what):
    """float[:, ::1] of the pyx: float32, 2-D, of the frame's shape (ValueError otherwise)."""
    arr = np.asarray(a)
    if arr.dtype != np.float32 or arr.ndim != 2:
        raise ValueError("%s must be a float32 array of shape [num_classes, num_nodes]" % what)
    if arr.shape[0] != shape[0]:
        raise ValueError("The first dimension of array should match the number of classes {}".format(shape[0]))
    if arr.shape[1] != shape[1]:
        raise ValueError("The second dimension of array should match the number of nodes {}".format(shape[1]))
    return np.ascontiguousarray(arr)


class SimpleCRFFrame(object):
    """One time frame of a SimpleCRF (csimple_crf.pyx:61-240).  It keeps its CRF alive (the pyx's parent_crf) and finds its frame by
    time on every call: a frame object whose time has been popped raises IndexError instead of touching freed memory."""

    def __init__(self, parent_crf, time):
        self.parent_crf = parent_crf
        self._time = int(time)

    @property
    def _h(self):
        return self.parent_crf._frame_handle(self._time)

    @property
    def time(self):
        return self._time

    @property
    def num_nodes(self):
        return self.parent_crf._num_nodes

    @property
    def num_classes(self):
        return self.parent_crf._num_classes

    @property
    def space_size(self):
        return self.num_classes * self.num_nodes

    def _fresh_buffer(self):
        return np.zeros([self.num_classes, self.num_nodes], dtype=np.float32)

    @property
    def unaries(self):
        out = self._fresh_buffer()
        B._check(_lib().fslic_hip_crf_frame_get_unary(self._h, out.ctypes.data))
        return out

    @unaries.setter
    def unaries(self, new_value):
        arr = _f32_2d(new_value, (self.num_classes, self.num_nodes), "unaries")
        B._check(_lib().fslic_hip_crf_frame_set_unary(self._h, arr.ctypes.data))

    def set_unbiased(self):
        B._check(_lib().fslic_hip_crf_frame_set_unbiased(self._h))

    def set_mask(self, classes, confidence):
        arr = np.asarray(classes)
        if arr.dtype != np.int32 or arr.ndim != 1:
            raise ValueError("classes must be a 1-D int32 array")
        if arr.shape[0] != self.num_nodes:
            raise ValueError("The dimension of class array should match the number of nodes {}".format(self.num_nodes))
        arr = np.ascontiguousarray(arr)
        B._check(_lib().fslic_hip_crf_frame_set_mask(self._h, arr.ctypes.data, float(confidence)))

    def set_proba(self, proba):
        arr = _f32_2d(proba, (self.num_classes, self.num_nodes), "proba")
        B._check(_lib().fslic_hip_crf_frame_set_proba(self._h, arr.ctypes.data))

    def get_inferred(self):
        out = self._fresh_buffer()
        B._check(_lib().fslic_hip_crf_frame_get_inferred(self._h, out.ctypes.data))
        return out

    def reset_inferred(self):
        B._check(_lib().fslic_hip_crf_frame_reset_inferred(self._h))

    # ---- clusters ----
    def get_clusters(self):
        """The frame's Cluster[num_nodes] block (structured array of CLUSTER_DTYPE); not part of the pyx surface."""
        out = np.zeros(self.num_nodes, B.CLUSTER_DTYPE)
        B._check(_lib().fslic_hip_crf_frame_get_clusters(self._h, out.ctypes.data))
        return out

    def set_clusters(self, clusters):
        """Set the Cluster[num_nodes] block as is (float centres and colours, no truncation); not part of the pyx surface."""
        cl = np.asarray(clusters)
        if cl.dtype != B.CLUSTER_DTYPE or cl.shape != (self.num_nodes,):
            raise ValueError("clusters must be a CLUSTER_DTYPE array of shape [{}]".format(self.num_nodes))
        cl = np.ascontiguousarray(cl)
        B._check(_lib().fslic_hip_crf_frame_set_clusters(self._h, cl.ctypes.data))

    def get_yxmrgb(self):                                                   # pyx:76-93
        cl = self.get_clusters()
        return [[float(c["y"]), float(c["x"]), int(c["num_members"]), float(c["r"]), float(c["g"]), float(c["b"])] for c in cl]

    def set_yxmrgb(self, yxmrgb):                                           # pyx:95-116: int32[:, ::1]
        arr = np.asarray(yxmrgb)
        if arr.dtype != np.int32 or arr.ndim != 2:
            raise ValueError("yxmrgb must be an int32 array of shape [num_nodes, 6]")
        if self.num_nodes != arr.shape[0]:
            raise ValueError("Expected the first dimension of yxmrgb to equal to {}".format(self.num_nodes))
        if 6 != arr.shape[1]:
            raise ValueError("Expected the second dimension of yxmrgb to equal to 6")
        cl = np.zeros(self.num_nodes, B.CLUSTER_DTYPE)
        cl["y"], cl["x"], cl["num_members"] = arr[:, 0], arr[:, 1], arr[:, 2].astype(np.uint32)
        cl["r"], cl["g"], cl["b"] = arr[:, 3], arr[:, 4], arr[:, 5]
        cl["number"] = np.arange(self.num_nodes, dtype=np.uint16)
        self.set_clusters(cl)

    # ---- neighbour lists ----
    def get_connectivity(self):                                             # pyx:118-125
        lib = _lib()
        off = np.zeros(self.num_nodes + 1, np.int64)
        B._check(lib.fslic_hip_crf_frame_get_connectivity(self._h, off.ctypes.data, None))
        idx = np.zeros(max(int(off[-1]), 1), np.uint32)
        B._check(lib.fslic_hip_crf_frame_get_connectivity(self._h, off.ctypes.data, idx.ctypes.data))
        return [[int(v) for v in idx[off[i]:off[i + 1]]] for i in range(self.num_nodes)]

    def set_connectivity(self, connectivity):                               # pyx:130-167
        if isinstance(connectivity, B.NodeConnectivity):
            num = np.ascontiguousarray(connectivity.num_neighbors, dtype=np.int32)
            nb = np.ascontiguousarray(connectivity.neighbors, dtype=np.uint32)
            if nb.ndim != 2 or num.ndim != 1 or num.shape[0] != nb.shape[0]:
                raise ValueError("malformed NodeConnectivity")
            if num.shape[0] > self.num_nodes:
                raise ValueError("Expected at most {} rows of connectivity".format(self.num_nodes))
            B._check(_lib().fslic_hip_crf_frame_set_connectivity(self._h, num.shape[0], num.ctypes.data,
                                                                  nb.ctypes.data if nb.size else None, nb.shape[1]))
            return
        if len(connectivity) != self.num_nodes:
            raise ValueError("Expected len(connectivity) to be {}".format(self.num_nodes))
        lengths = [len(neighbors) for neighbors in connectivity]          # TypeError for a row that is not a sequence, as in the pyx
        off = np.zeros(self.num_nodes + 1, np.int64)
        off[1:] = np.cumsum(lengths)
        idx = np.zeros(max(int(off[-1]), 1), np.uint32)
        k = 0
        for neighbors in connectivity:
            for neighbor in neighbors:
                v = int(neighbor) if isinstance(neighbor, (int, np.integer)) else neighbor.__index__()
                if v < 0 or v > 0xFFFFFFFF:
                    raise OverflowError("neighbour index out of range for uint32_t")
                idx[k] = v
                k += 1
        B._check(_lib().fslic_hip_crf_frame_set_connectivity_csr(self._h, self.num_nodes, off.ctypes.data, idx.ctypes.data))

    # ---- energies ----
    def spatial_pairwise_energy(self, node_i, node_j):                     # pyx:205-211
        if not 0 <= int(node_i) < self.num_nodes or not 0 <= int(node_j) < self.num_nodes:
            raise ValueError("node number is out of range")
        out = C.c_float()
        B._check(_lib().fslic_hip_crf_frame_spatial_energy(self._h, int(node_i), int(node_j), C.byref(out)))
        return out.value

    def temporal_pairwise_energy(self, node_i, other):                     # pyx:193-203
        if not isinstance(other, SimpleCRFFrame):
            raise TypeError("not a crf frame")
        if not 0 <= int(node_i) < self.num_nodes:
            raise ValueError("node number is out of range")
        out = C.c_float()
        B._check(_lib().fslic_hip_crf_frame_temporal_energy(self._h, other._h, int(node_i), C.byref(out)))
        return out.value


def _param_property(name):
    def get(self):
        return getattr(self._get_params(), name)

    def set_(self, value):
        p = self._get_params()
        setattr(p, name, float(value))
        B._check(_lib().fslic_hip_crf_set_params(self._h, C.byref(p)))
    return property(get, set_)


class SimpleCRF(object):
    """csimple_crf.SimpleCRF (csimple_crf.pyx:244-356) with inference on the GPU.  `device` picks the engine (the process-wide
    default_engine of that GPU), taken at the first inference(); everything else works without a GPU."""

    def __init__(self, num_classes, num_nodes, device=0):
        num_classes, num_nodes = int(num_classes), int(num_nodes)
        if num_classes < 0 or num_nodes < 0:
            raise OverflowError("can't convert negative value to size_t")
        lib = _lib()
        h = C.c_void_p()
        B._check(lib.fslic_hip_crf_new(num_classes, num_nodes, C.byref(h)))
        self._h = h
        self._num_classes = num_classes
        self._num_nodes = num_nodes
        self.device = int(device)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib().fslic_hip_crf_free(h)
            except Exception:
                pass
            self._h = None

    def copy(self):
        """A deep copy (frames, unaries, q, params); not part of the pyx surface."""
        h = C.c_void_p()
        B._check(_lib().fslic_hip_crf_copy(self._h, C.byref(h)))
        new = SimpleCRF.__new__(SimpleCRF)
        new._h, new._num_classes, new._num_nodes, new.device = h, self._num_classes, self._num_nodes, self.device
        return new

    def _get_params(self):
        p = _Params()
        B._check(_lib().fslic_hip_crf_get_params(self._h, C.byref(p)))
        return p

    spatial_w = _param_property("spatial_w")
    spatial_srgb = _param_property("spatial_srgb")
    spatial_sxy = _param_property("spatial_sxy")
    temporal_w = _param_property("temporal_w")
    temporal_srgb = _param_property("temporal_srgb")
    spatial_smooth_w = _param_property("spatial_smooth_w")
    spatial_smooth_sxy = _param_property("spatial_smooth_sxy")

    def get_compat(self, cls):
        out = C.c_float()
        B._check(_lib().fslic_hip_crf_get_compat(self._h, int(cls), C.byref(out)))
        return out.value

    def set_compat(self, cls, value):
        """SimpleCRF::compat_by_class[cls] (src/simple-crf.hpp:77; simple_crf_set_compat); not part of the pyx surface."""
        B._check(_lib().fslic_hip_crf_set_compat(self._h, int(cls), float(value)))

    @property
    def first_time(self):
        return _lib().fslic_hip_crf_first_time(self._h)

    @property
    def last_time(self):
        return _lib().fslic_hip_crf_last_time(self._h)

    @property
    def num_frames(self):
        return _lib().fslic_hip_crf_num_frames(self._h)

    @property
    def space_size(self):
        return self._num_classes * self._num_nodes

    def _frame_handle(self, time):
        h = C.c_void_p()
        rc = _lib().fslic_hip_crf_frame(self._h, int(time), C.byref(h))
        if rc == B.FSLIC_E_INVALID:
            raise IndexError("Time out of range")
        B._check(rc)
        return h

    def get_frame(self, time):                                              # pyx:318-322; IndexError for a missing time
        self._frame_handle(time)
        return SimpleCRFFrame(self, time)

    def push_frame(self):
        h = C.c_void_p()
        B._check(_lib().fslic_hip_crf_push_frame(self._h, C.byref(h)))
        return SimpleCRFFrame(self, _lib().fslic_hip_crf_frame_time(h))

    def pop_frame(self):
        return _lib().fslic_hip_crf_pop_frame(self._h)

    def push_slic_frame(self, slic, knn=None):
        """Push a frame built from a finished Slic run: its clusters, its neighbour lists, unbiased unaries.

        Differs from csimple_crf.pyx:324-332 on purpose: there the clusters go through `to_yxmrgb()`, which returns a float array that
        `set_yxmrgb` (int32 only) refuses, so the reference's version cannot run.  Here `slic.slic_model.cluster_array` (the Cluster[K]
        block) is set as is -- float centres and colours, no integer truncation.  The neighbour lists are
        `slic.slic_model.get_connectivity(slic.last_assignment)`, or `get_knn_connectivity(..., knn)` when knn is given."""
        frame = self.push_frame()
        model = slic.slic_model
        frame.set_clusters(model.cluster_array)
        if knn is None:
            frame.set_connectivity(model.get_connectivity(slic.last_assignment))
        else:
            frame.set_connectivity(model.get_knn_connectivity(slic.last_assignment, knn))
        frame.set_unbiased()
        return frame

    def initialize(self):
        B._check(_lib().fslic_hip_crf_initialize(self._h))

    def inference(self, max_iter):
        max_iter = int(max_iter)
        if max_iter < 0:
            raise OverflowError("can't convert negative value to size_t")
        eng = B.default_engine(self.device)._h if max_iter > 0 and self.num_frames > 0 else None     # (no GPU needed otherwise)
        B._check(_lib().fslic_hip_crf_inference(self._h, eng, max_iter))
