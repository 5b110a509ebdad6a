"""CPU test: what every stream entry of the C ABI refuses, with which words and in which order.  No kernel is launched.

The stream entries are the 33 fslic_hip_* functions that take (device, stream, ...) and own no buffer, and their ten *_workspace_size
companions (csrc/*api.cpp except capi.cpp, on csrc/streamapi.h).  For each of them TABLE holds a set of valid arguments -- small
sizes, 0x1000 for every pointer -- and the entry's checks in the order of its source: (site, the arguments that violate it, the
exact bytes of fslic_hip_last_error()).  Row i of an entry is built from that list: check i's violation on top of the violation
of EVERY later check, an earlier check's arguments winning where two name the same one.  So a row is refused with check i's words
only if check i comes before all the others it violates, and one row pins both the text and the order.  Where two checks cannot be
violated at once (they need different values of one argument, or the later one is only looked at once the earlier one holds) a
comment next to the entry says so.  Entries that answer FSLIC_OK before any HIP call (nothing to do) have a row for that too.

The texts were recorded from the library as it was before these entries were restated on streamapi.h's shared checks, and a
`site` names the `fail(FSLIC_E_INVALID` of that source, numbered per file in source order ("merge:5": the fifth one of
mergeapi.cpp; "stream:" the ones of streamapi.h).  The ten *api.cpp files held 134 of them (SITES); the table reaches every one.
streamapi.h's "no such HIP device" needs a HIP call and is the one refusal that is not here.

No call here passes every check.  Should a row ever do so by mistake, the device it names does not exist: DeviceScope then refuses
it ("no such HIP device") before a bogus pointer is touched."""
import ctypes as C

import pytest

from fast_slic_amd import _binding as B

P = C.c_void_p(0x1000)
ODD = C.c_void_p(0x1001)                      # aligned to nothing
NUL = None
DEVICE = 0x7FFFFFFF                           # passes `device >= 0`; see the last paragraph above
SIZE = C.c_size_t()
BYTES = C.byref(SIZE)                         # where a *_workspace_size entry writes
BIG = 1 << 40                                 # a workspace of this many bytes is large enough for the sizes used here
STRIDES = C.cast(P, C.POINTER(C.c_longlong))
NULL_ARG = b"NULL pointer argument"

# the number of `fail(FSLIC_E_INVALID` in each of the ten files at the commit the texts were recorded from
SITES = dict(pool=12, rag=12, compare=12, crf=15, soft=13, connect=8, merge=24, region=14, ingest=11, aggregate=13)


# ---- checks that several entries share ----
def label_map(label_type="label_type"):       # streamapi.h check_label_map.  H = 0 leaves no way to too many pixels or frames, an N = 0 ahead of it none to too many frames
    return [("stream:2", dict(H=0), b"H and W must be positive"),
            ("stream:3", dict(H=1 << 16, W=1 << 15), b"H * W must be below 2^31"),
            ("stream:4", dict(N=1 << 12, H=1 << 15, W=1 << 14), b"too many frames"),
            ("stream:1", {label_type: 3}, b"unknown label type")]


def pair_table(device=True, frames=True):     # streamapi.h check_pair_table.  N = 0 leaves no way to N * capacity >= 2^40
    checks = [("stream:5", dict(device=-1), b"device must be >= 0"), ("stream:6", dict(N=0), b"N must be positive")]
    return checks[0 if device else 1:2 if frames else 1] + [
        ("stream:7", dict(capacity=1 << 32), b"capacity must be a power of two in [64, 2^31]"),
        ("stream:8", dict(N=1 << 12, capacity=1 << 31), b"N * capacity must be below 2^40")]


def pool_common(device=True, reduce=True):    # N = 0 leaves no way to N * C * K >= 2^40
    checks = [("pool:1", dict(device=-1), b"device must be >= 0"), ("pool:2", dict(N=0), b"N and C must be positive"),
              ("pool:3", dict(K=65535), b"K must be in [1, 65534]"), ("pool:4", dict(reduce=3), b"unknown reduce"),
              ("pool:5", dict(N=1 << 13, C=1 << 13, K=65534), b"N * C * K must be below 2^40")]
    return [c for c in checks[0 if device else 1:] if reduce or c[0] != "pool:4"]


def rag_tables(device=True, nodes=True):
    checks = pair_table(device) + [("rag:1", dict(K=0), b"K must be in [1, 65534]"), ("rag:2", dict(C=5), b"C must be in [0, 4] (0: no image)")]
    return [c for c in checks if nodes or c[0] != "rag:1"]


def crf_sizes(entries=True, classes=True):    # N = 0 leaves no way to N * C * K >= 2^31
    big = dict(N=1 << 11, C=1 << 10, K=1 << 10) if classes else dict(N=1 << 16, K=1 << 15)
    checks = [("crf:1", dict(N=0), b"N, C and K must be positive"), ("crf:2", dict(nnz=1 << 31), b"nnz must be in [0, 2^31)"),
              ("crf:3", big, b"N * C * K and N * K + 1 must be below 2^31")]
    return [c for c in checks if entries or c[0] != "crf:2"]


def crf_call(max_iter=True, classes=True):
    return ([("crf:4", dict(device=-1), b"device must be >= 0")] + crf_sizes(classes=classes) + [("crf:5", dict(temporal=2), b"temporal must be 0 or 1")]
            + ([("crf:6", dict(max_iter=-1), b"max_iter must be >= 0")] if max_iter else []))


def crf_workspace(needed):                    # the alignment is the workspace pointer's: the NULL check ahead of it is violated by another pointer
    return [("crf:7", dict(workspace=C.c_void_p(0x1008)), b"workspace must be 16-byte aligned"),
            ("crf:8", dict(workspace_bytes=0), b"workspace too small: %d bytes needed" % needed)]


def crf_sweeps(needed):
    return crf_call() + [("crf:9", dict(compat=NUL, members=NUL, offsets=NUL, unaries=NUL), NULL_ARG)] + crf_workspace(needed)


def soft_checks(null):
    # H = 0 leaves no way to H * W >= 2^31; a grid below 1 x 1 is larger than 65534 cells only with both sides negative
    return [("soft:1", dict(device=-1), b"device must be >= 0"), ("soft:2", dict(C=0), b"N and C must be positive"),
            ("soft:3", dict(H=0), b"H and W must be positive"), ("soft:4", dict(H=1 << 16, W=1 << 15), b"H * W must be below 2^31"),
            ("soft:5", dict(gh=-256, gw=-256), b"the grid must be 1 <= gh <= H and 1 <= gw <= W"),
            ("soft:6", dict(H=256, W=256, gh=256, gw=256), b"gh * gw must be at most 65534"),
            ("soft:7", dict(N=1 << 23, H=256, W=256), b"too many frames"),
            ("soft:8", dict(N=1 << 16, H=256, W=256, gh=255, gw=255), b"N * gh * gw * ceil(C / 16) must be below 2^31"), null]


def connect_map(label_type=True):             # N = 0 and H = 0 leave no way to N * H * W >= 2^31
    return [("connect:1", dict(N=0), b"N must be positive"), ("connect:2", dict(H=0), b"H and W must be positive"),
            ("connect:3", dict(H=1 << 16, W=1 << 15), b"N * H * W must be below 2^31")] + ([("stream:1", dict(label_type=3), b"unknown label type")] if label_type else [])


def run_connect(min_size=True):
    return ([("connect:4", dict(device=-1), b"device must be >= 0")] + connect_map() + ([("connect:5", dict(min_size=-1), b"min_size must be >= 0")] if min_size else [])
            + [("connect:6", dict(labels=NUL, workspace=NUL), NULL_ARG), ("connect:7", dict(workspace_bytes=0), b"workspace too small: 336 bytes needed")])


def merge_nodes(device=True):                 # N = 0 leaves no way to N * K >= 2^31
    return [("merge:1", dict(device=-1), b"device must be >= 0"), ("merge:2", dict(N=0), b"N must be positive"),
            ("merge:3", dict(K=65535), b"K must be in [1, 65534]"), ("merge:4", dict(N=1 << 16, K=1 << 15), b"N * K must be below 2^31")][0 if device else 1:]


MERGE_EDGES = [("merge:5", dict(E=1 << 31), b"E must be in [0, 2^31)"), ("merge:6", dict(offsets=NUL, edge_index=NUL), NULL_ARG)]


def region_cells(K="K"):                      # N = 0 leaves no way to N * C * K >= 2^31
    return [("region:1", dict(N=0), b"N must be positive"), ("region:2", dict(C=0), b"C must be positive"),
            ("region:3", {K: 65535}, b"%s must be in [1, 65534]" % K.encode()), ("region:4", {"N": 1 << 16, K: 1 << 15}, b"N * C * %s must be below 2^31" % K.encode())]


def aggregate_call():                         # N = 0 leaves no way to N * C * K >= 2^31
    return [("aggregate:1", dict(device=-1), b"device must be >= 0"), ("aggregate:2", dict(N=0), b"N must be positive"),
            ("aggregate:3", dict(C=0), b"C must be positive"), ("aggregate:4", dict(K=65535), b"K must be in [1, 65534]"),
            ("aggregate:5", dict(N=1 << 16, K=1 << 15), b"N * C * K must be below 2^31"), ("aggregate:6", dict(nnz=-1), b"nnz must be in [0, 2^31)")]


# a weight is refused with the mean and the max, so the two checks behind it see none; the max and the mean are one argument
AGGREGATE_REDUCE = [("aggregate:7", dict(reduce=3), b"reduce must be 0 (sum), 1 (mean) or 2 (max)"),
                    ("aggregate:8", dict(reduce=1, weight=P), b"a weight goes with reduce 0 (sum) only"),
                    ("aggregate:9", dict(reduce=2, weight=NUL, argmax=NUL), b"reduce 2 (max) needs argmax"),
                    ("aggregate:10", dict(reduce=1, weight=NUL, degree=NUL), b"reduce 1 (mean) needs degree")]

# ---- the valid arguments, in the order of include/fslic_hip.h ----
SWEEP = dict(device=DEVICE, stream=NUL, N=2, C=3, K=5, temporal=1, max_iter=2)
LISTS = dict(members=P, offsets=P, indices=P, nnz=14)
WS = dict(workspace=P, workspace_bytes=BIG)
INFERENCE = dict(SWEEP, params=P, compat=P, yxrgb=P, **LISTS, unaries=P, q0=P, q_out=P, **WS)
BACKWARD = dict(SWEEP, params=P, compat=P, yxrgb=P, **LISTS, t_offsets=P, t_entries=P, t_rows=P, unaries=P, q_all=P, grad_q=P, grad_unaries=P, grad_q0=P,
                grad_compat=P, **WS)
INFERENCE_ENERGIES = dict(SWEEP, compat=P, **LISTS, edge=P, links=P, unaries=P, q0=P, q_out=P, **WS)
BACKWARD_ENERGIES = dict(SWEEP, compat=P, **LISTS, edge=P, links=P, t_offsets=P, t_entries=P, t_rows=P, unaries=P, q_all=P, grad_q=P, grad_unaries=P,
                         grad_q0=P, grad_compat=P, grad_edge=P, grad_links=P, **WS)
SOFT = dict(device=DEVICE, stream=NUL, N=2, C=3, H=4, W=5, gh=2, gw=2)
CONNECT = dict(device=DEVICE, stream=NUL, N=2, H=4, W=5, labels=P, label_type=1)
GRAPH = dict(device=DEVICE, stream=NUL, N=2, K=5, E=7, edge_index=P, offsets=P)
AGGREGATE = dict(device=DEVICE, stream=NUL, N=2, C=3, K=5, nnz=14)

# (entry, valid arguments, checks in source order, argument sets answered with FSLIC_OK before any HIP call)
TABLE = [
    # ---- poolapi.cpp ----
    ("fslic_hip_pool_workspace_size", dict(N=2, C=3, K=5, reduce=0, bytes=BYTES),
     [("pool:6", dict(bytes=NUL), NULL_ARG)] + pool_common(device=False), []),
    ("fslic_hip_pool", dict(device=DEVICE, stream=NUL, N=2, C=3, H=4, W=5, K=5, reduce=0, features=P, labels=P, label_type=0, **WS),
     pool_common() + label_map() + [("pool:7", dict(features=NUL, labels=NUL, workspace=NUL), NULL_ARG),
                                    ("pool:8", dict(workspace_bytes=0), b"workspace too small: 1720 bytes needed")], []),
    # an argmax is refused unless the reduction is the max: any other reduce, the unknown one included, violates that check as well
    ("fslic_hip_pool_finalize", dict(device=DEVICE, stream=NUL, N=2, C=3, K=5, reduce=0, workspace=P, workspace_bytes=BIG, values=P, counts=P, argmax=NUL),
     pool_common() + [("pool:9", dict(workspace=NUL, values=NUL), NULL_ARG), ("pool:10", dict(argmax=P), b"argmax needs reduce == FSLIC_POOL_MAX"),
                      ("pool:11", dict(workspace_bytes=0), b"workspace too small")], []),
    # (the reduction is not an argument here: "unknown reduce" cannot be reached)
    ("fslic_hip_unpool", dict(device=DEVICE, stream=NUL, N=2, C=3, H=4, W=5, K=5, values=P, labels=P, label_type=0, argmax=NUL, fill=0.0, out=P),
     pool_common(reduce=False) + label_map() + [("pool:12", dict(values=NUL, labels=NUL, out=NUL), NULL_ARG)], []),
    # ---- ragapi.cpp ----
    ("fslic_hip_rag_workspace_size", dict(N=2, K=5, C=3, capacity=64, bytes=BYTES),
     [("rag:3", dict(bytes=NUL), NULL_ARG)] + rag_tables(device=False), []),
    # C = 5 is refused by itself; with it, "no image" is the violation of the check that image and C agree
    ("fslic_hip_rag_accumulate", dict(device=DEVICE, stream=NUL, N=2, H=4, W=5, K=5, connectivity=8, labels=P, label_type=0, image=P, C=3, capacity=64, **WS),
     rag_tables() + label_map() + [("rag:4", dict(H=1 << 15, W=1 << 14), b"H * W must be below 2^29"), ("rag:5", dict(connectivity=5), b"connectivity must be 4 or 8"),
                                   ("rag:6", dict(labels=NUL, workspace=NUL), NULL_ARG), ("rag:7", dict(image=NUL), b"an image needs C in [1, 4], no image needs C == 0"),
                                   ("rag:8", dict(workspace_bytes=0), b"workspace too small: 4128 bytes needed")], []),
    # (K is not an argument here.)  C = 5 and C = 0 are one argument: the row of "C must be in [0, 4]" leaves "contrast needs C" valid
    ("fslic_hip_rag_compact", dict(device=DEVICE, stream=NUL, N=2, C=3, capacity=64, workspace=P, workspace_bytes=BIG, keys=P, boundary=P, contrast=P, max_edges=10),
     rag_tables(nodes=False) + [("rag:9", dict(workspace=NUL, keys=NUL, boundary=NUL), NULL_ARG), ("rag:10", dict(C=0), b"contrast needs C in [1, 4]"),
                                ("rag:11", dict(max_edges=-1), b"max_edges must be >= 0"), ("rag:12", dict(workspace_bytes=0), b"workspace too small")], []),
    # ---- compareapi.cpp ----
    ("fslic_hip_overlap_workspace_size", dict(N=2, capacity=64, bytes=BYTES), [("compare:1", dict(bytes=NUL), NULL_ARG)] + pair_table(device=False), []),
    ("fslic_hip_overlap_accumulate", dict(device=DEVICE, stream=NUL, N=2, H=4, W=5, K=5, M=6, labels=P, label_type=0, other=P, other_type=2, capacity=64, **WS),
     pair_table() + label_map() + [("stream:1", dict(other_type=-1), b"unknown label type"), ("compare:2", dict(K=0), b"K must be in [1, 65534]"),
                                   ("compare:3", dict(M=65535), b"M must be in [1, 65534]"), ("compare:4", dict(labels=NUL, other=NUL, workspace=NUL), NULL_ARG),
                                   ("compare:5", dict(workspace_bytes=0), b"workspace too small: 1056 bytes needed")], []),
    ("fslic_hip_overlap_compact", dict(device=DEVICE, stream=NUL, N=2, capacity=64, workspace=P, workspace_bytes=BIG, keys=P, count=P, max_pairs=10),
     pair_table() + [("compare:6", dict(workspace=NUL, keys=NUL, count=NUL), NULL_ARG), ("compare:7", dict(max_pairs=-1), b"max_pairs must be >= 0"),
                     ("compare:8", dict(workspace_bytes=0), b"workspace too small")], []),
    ("fslic_hip_boundary_match", dict(device=DEVICE, stream=NUL, N=2, H=4, W=5, labels=P, label_type=0, other=P, other_type=2, tolerance=2, counts=P),
     [("compare:9", dict(device=-1), b"device must be >= 0"), ("compare:10", dict(N=0), b"N must be positive")] + label_map()
     + [("stream:1", dict(other_type=-1), b"unknown label type"), ("compare:11", dict(tolerance=16), b"tolerance must be in [0, 15]"),
        ("compare:12", dict(labels=NUL, other=NUL, counts=NUL), NULL_ARG)], []),
    # ---- crfapi.cpp ----
    ("fslic_hip_crf_tensor_workspace_size", dict(N=2, C=3, K=5, nnz=14, bytes=BYTES), [("crf:10", dict(bytes=NUL), NULL_ARG)] + crf_sizes(), []),
    ("fslic_hip_crf_tensor_inference", INFERENCE, crf_sweeps(480), []),
    ("fslic_hip_crf_tensor_grad_workspace_size", dict(N=2, C=3, K=5, nnz=14, backward=1, with_compat=1, bytes=BYTES),
     [("crf:11", dict(bytes=NUL), NULL_ARG)] + crf_sizes() + [("crf:12", dict(backward=2, with_compat=-1), b"backward and with_compat must be 0 or 1")], []),
    ("fslic_hip_crf_tensor_inference_saved", INFERENCE, crf_sweeps(352), []),
    ("fslic_hip_crf_tensor_backward", BACKWARD, crf_sweeps(624), []),
    # (C and max_iter are not arguments of the two entries of the energies)
    ("fslic_hip_crf_tensor_energies", dict(device=DEVICE, stream=NUL, N=2, K=5, temporal=1, params=P, yxrgb=P, **LISTS, edge=P, links=P),
     crf_call(max_iter=False, classes=False) + [("crf:13", dict(params=NUL, yxrgb=NUL, members=NUL, offsets=NUL, links=NUL), NULL_ARG)], []),
    ("fslic_hip_crf_tensor_energies_backward_workspace_size", dict(N=2, K=5, bytes=BYTES),
     [("crf:14", dict(bytes=NUL), NULL_ARG)] + crf_sizes(entries=False, classes=False), []),
    ("fslic_hip_crf_tensor_energies_backward", dict(device=DEVICE, stream=NUL, N=2, K=5, temporal=1, params=P, yxrgb=P, offsets=P, indices=P, nnz=14, grad_edge=P,
                                                    grad_links=P, grad_params=P, **WS),
     crf_call(max_iter=False, classes=False) + [("crf:15", dict(params=NUL, yxrgb=NUL, offsets=NUL, grad_params=NUL), NULL_ARG)] + crf_workspace(64), []),
    ("fslic_hip_crf_tensor_inference_energies", INFERENCE_ENERGIES, crf_sweeps(480), []),
    ("fslic_hip_crf_tensor_inference_saved_energies", INFERENCE_ENERGIES, crf_sweeps(352), []),
    ("fslic_hip_crf_tensor_backward_energies", BACKWARD_ENERGIES, crf_sweeps(624), []),
    # ---- softapi.cpp ----
    ("fslic_hip_soft_assign", dict(SOFT, features=P, centres=P, q=P), soft_checks(("soft:9", dict(features=NUL, centres=NUL, q=NUL), NULL_ARG)), []),
    ("fslic_hip_soft_assign_backward", dict(SOFT, features=P, centres=P, q=P, grad_q=P, grad_d=P, grad_features=P),
     soft_checks(("soft:10", dict(features=NUL, grad_features=NUL), NULL_ARG)), []),
    ("fslic_hip_soft_pool", dict(SOFT, features=P, q=P, centres=P, sums=P, weights=P), soft_checks(("soft:11", dict(features=NUL, q=NUL, sums=NUL), NULL_ARG)), []),
    ("fslic_hip_soft_unpool", dict(SOFT, values=P, q=P, out=P), soft_checks(("soft:12", dict(values=NUL, q=NUL, out=NUL), NULL_ARG)), []),
    ("fslic_hip_soft_dot", dict(SOFT, a=P, b=P, bias=P, out=P), soft_checks(("soft:13", dict(a=NUL, b=NUL, out=NUL), NULL_ARG)), []),
    # ---- connectapi.cpp ----
    # (the label type is not an argument of the size entry, min_size not one of the components')
    ("fslic_hip_connect_workspace_size", dict(N=2, H=4, W=5, bytes=BYTES), [("connect:8", dict(bytes=NUL), NULL_ARG)] + connect_map(label_type=False), []),
    ("fslic_hip_connected_components", dict(CONNECT, components=P, counts=P, **WS), run_connect(min_size=False), []),
    ("fslic_hip_connect_enforce", dict(CONNECT, min_size=3, out=P, counts=P, **WS), run_connect(), []),
    # ---- mergeapi.cpp ----
    ("fslic_hip_merge_best_workspace_size", dict(N=2, K=5, bytes=BYTES), [("merge:7", dict(bytes=NUL), NULL_ARG)] + merge_nodes(device=False), []),
    ("fslic_hip_merge_best_edges", dict(GRAPH, weight=P, has_threshold=0, threshold=0.0, join=P, **WS),
     merge_nodes() + MERGE_EDGES + [("merge:8", dict(weight=NUL, join=NUL), NULL_ARG), ("merge:9", dict(workspace=NUL), NULL_ARG),
                                    ("merge:10", dict(workspace_bytes=0), b"workspace too small: 80 bytes needed")],
     [dict(E=0), dict(E=0, edge_index=NUL, weight=NUL, join=NUL)]),
    ("fslic_hip_merge_components_workspace_size", dict(N=2, K=5, bytes=BYTES), [("merge:11", dict(bytes=NUL), NULL_ARG)] + merge_nodes(device=False), []),
    ("fslic_hip_merge_components", dict(GRAPH, join=P, members=NUL, members_type=1, mapping=P, counts=P, **WS),
     merge_nodes() + MERGE_EDGES + [("merge:12", dict(join=NUL), NULL_ARG), ("merge:13", dict(members=P, members_type=0), b"members must be int32 or int64"),
                                    ("merge:14", dict(mapping=NUL, counts=NUL, workspace=NUL), NULL_ARG),
                                    ("merge:15", dict(workspace_bytes=0), b"workspace too small: 112 bytes needed")], []),
    # H = 0 leaves no way to N * H * W >= 2^31; the alignment is `out`'s, so the NULL check ahead of it is violated by the other pointers
    ("fslic_hip_merge_labels", dict(device=DEVICE, stream=NUL, N=2, H=4, W=5, K=5, labels=P, label_type=0, mapping=P, out=P),
     merge_nodes() + [("merge:16", dict(H=0), b"H and W must be positive"), ("merge:17", dict(H=1 << 16, W=1 << 15), b"N * H * W must be below 2^31"),
                      ("stream:1", dict(label_type=3), b"unknown label type"), ("merge:18", dict(labels=NUL, mapping=NUL), NULL_ARG),
                      ("merge:19", dict(out=C.c_void_p(0x1002)), b"out must be 4-byte aligned")], []),
    # (the pair table's own device and N checks stand behind check_nodes' and cannot be reached)
    ("fslic_hip_merge_contract_accumulate", dict(device=DEVICE, stream=NUL, N=2, K=5, K2=4, E=7, edge_index=P, offsets=P, boundary=P, contrast=P, C=3, mapping=P,
                                                 capacity=64, **WS),
     merge_nodes() + pair_table(device=False, frames=False) + MERGE_EDGES
     + [("merge:20", dict(K2=0), b"K2 must be in [1, 65534]"), ("merge:21", dict(C=5), b"C must be in [0, 4] (0: no contrast)"),
        ("merge:22", dict(contrast=NUL), b"contrast needs C in [1, 4], no contrast needs C == 0"), ("merge:23", dict(boundary=NUL, mapping=NUL, workspace=NUL), NULL_ARG),
        ("merge:24", dict(workspace_bytes=0), b"workspace too small: 4128 bytes needed")], []),
    # ---- regionapi.cpp ----
    ("fslic_hip_region_sums_workspace_size", dict(N=2, C=3, K2=4, bytes=BYTES), [("region:6", dict(bytes=NUL), NULL_ARG)] + region_cells("K2"), []),
    # check_cells runs for K, then for K2: its N and C checks cannot be reached the second time.  counts_type is looked at only with counts
    ("fslic_hip_region_sums", dict(device=DEVICE, stream=NUL, N=2, C=3, K=5, K2=4, values=P, mapping=P, counts=P, counts_type=1, sums=P, counts_out=P, **WS),
     [("region:7", dict(device=-1), b"device must be >= 0")] + region_cells() + region_cells("K2")[2:]
     + [("region:5", dict(counts_type=0), b"counts must be int32 or int64"), ("region:8", dict(counts_out=NUL), b"counts and counts_out go together"),
        ("region:9", dict(values=NUL, mapping=NUL, sums=NUL, workspace=NUL), NULL_ARG), ("region:10", dict(workspace_bytes=0), b"workspace too small: 1344 bytes needed")], []),
    ("fslic_hip_region_edge_weights", dict(device=DEVICE, stream=NUL, N=2, C=3, K=5, E=7, edge_index=P, offsets=P, sums=P, counts=P, counts_type=1, mode=0, weight=P),
     [("region:11", dict(device=-1), b"device must be >= 0")] + region_cells()
     + [("region:5", dict(counts_type=0), b"counts must be int32 or int64"), ("region:12", dict(E=1 << 31), b"E must be in [0, 2^31)"),
        ("region:13", dict(mode=2), b"mode must be 0 (mean) or 1 (ward)"), ("region:14", dict(offsets=NUL, sums=NUL, counts=NUL, edge_index=NUL, weight=NUL), NULL_ARG)],
     [dict(E=0), dict(E=0, edge_index=NUL, weight=NUL)]),
    # ---- ingestapi.cpp ----
    # the two alignments are src's and out's, so the NULL check ahead of them is violated by `strides`.  H = 0 leaves no way to H * W >= 2^31.  An
    # unknown source type counts as two bytes an element.  A pitch that is no multiple of 16 can be above 2^33 as well
    ("fslic_hip_pack_rgb", dict(device=DEVICE, stream=NUL, N=2, H=4, W=5, src=P, src_type=3, strides=STRIDES, scale=1.0, out=P, pitch=64),
     [("ingest:1", dict(device=-1), b"device must be >= 0"), ("ingest:2", dict(strides=NUL), NULL_ARG), ("ingest:3", dict(H=0), b"N, H and W must be positive"),
      ("ingest:4", dict(H=1 << 16, W=1 << 15), b"H * W must be below 2^31"), ("ingest:5", dict(src_type=4), b"unknown source type"),
      ("ingest:6", dict(pitch=(1 << 33) + 8), b"pitch must be at least H * W * 3 and a multiple of 16"), ("ingest:7", dict(pitch=(1 << 33) + 16), b"pitch must be at most 2^33"),
      ("ingest:8", dict(scale=float("inf")), b"scale must be finite"), ("ingest:9", dict(out=ODD), b"out is not 4-byte aligned"),
      ("ingest:10", dict(src=ODD), b"src is not aligned to its element type"), ("ingest:11", dict(N=1 << 10, pitch=1 << 33), b"too many frames")], []),
    # ---- aggregateapi.cpp ----
    ("fslic_hip_aggregate_forward", dict(AGGREGATE, reduce=0, offsets=P, indices=P, weight=P, values=P, out=P, argmax=P, degree=P),
     aggregate_call() + AGGREGATE_REDUCE + [("aggregate:11", dict(offsets=NUL, values=NUL, out=NUL, indices=NUL), NULL_ARG)], []),
    ("fslic_hip_aggregate_backward_values", dict(AGGREGATE, reduce=0, t_offsets=P, t_entries=P, t_rows=P, weight=P, argmax=P, degree=P, grad_out=P, grad_values=P),
     aggregate_call() + AGGREGATE_REDUCE + [("aggregate:12", dict(t_offsets=NUL, grad_out=NUL, grad_values=NUL, t_entries=NUL, t_rows=NUL), NULL_ARG)], []),
    ("fslic_hip_aggregate_backward_weight", dict(AGGREGATE, rows=P, indices=P, values=P, grad_out=P, grad_weight=P),
     aggregate_call() + [("aggregate:13", dict(values=NUL, grad_out=NUL, rows=NUL, indices=NUL, grad_weight=NUL), NULL_ARG)],
     [dict(nnz=0), dict(nnz=0, rows=NUL, indices=NUL, grad_weight=NUL)]),
]


def rows_of(valid, checks):
    """Row i: the valid arguments, then the violations of the checks from the last down to check i, so that an earlier one's values win."""
    for i, (site, _, text) in enumerate(checks):
        args = dict(valid)
        for _, bad, _ in reversed(checks[i:]):
            assert set(bad) <= set(valid), (site, bad)
            args.update(bad)
        yield site, args, text


REFUSALS = [pytest.param(name, args, text, id="%s-%d-%s" % (name[len("fslic_hip_"):], i, site))
            for name, valid, checks, _ in TABLE for i, (site, args, text) in enumerate(rows_of(valid, checks))]
NOTHING_TO_DO = [pytest.param(name, dict(valid, **kw), id="%s-%d" % (name[len("fslic_hip_"):], i))
                 for name, valid, _, oks in TABLE for i, kw in enumerate(oks)]


def lib():
    return B.load_library()


def test_the_table_holds_every_stream_entry():
    first = B.EXPORTS.index("fslic_hip_pool_workspace_size")      # the stream entries are the ones declared from here on
    names = [name for name, _, _, _ in TABLE]
    assert names == B.EXPORTS[first:] and len(names) == 43 and sum(n.endswith("_workspace_size") for n in names) == 10
    for name, valid, _, _ in TABLE:
        assert len(valid) == len(dict((n, a) for n, _, a in B.SIGNATURES)[name]) and hasattr(lib(), name), name


def test_the_table_reaches_every_site():
    assert sum(SITES.values()) == 134
    reached = {site for _, _, checks, _ in TABLE for site, _, _ in checks if not site.startswith("stream:")}
    assert reached == {"%s:%d" % (f, i + 1) for f, n in SITES.items() for i in range(n)}
    assert {site for _, _, checks, _ in TABLE for site, _, _ in checks if site.startswith("stream:")} == {"stream:%d" % i for i in range(1, 9)}


@pytest.mark.parametrize("name,args,text", REFUSALS)
def test_refused_with_these_words(name, args, text):
    assert (getattr(lib(), name)(*args.values()), lib().fslic_hip_last_error()) == (B.FSLIC_E_INVALID, text)


@pytest.mark.parametrize("name,args", NOTHING_TO_DO)
def test_nothing_to_do_is_ok_before_any_hip_call(name, args):
    assert getattr(lib(), name)(*args.values()) == B.FSLIC_OK
