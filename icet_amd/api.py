"""Host-side mirror of the reference interface for the accelerated path, on top of the C ABI.

The reference exposes exactly one operator for this path: the constructor of ``class ICET``
(/root/reference/include/icet.h:38-40, body src/icet.cpp:29-63), which *is* the solve; callers then
read the public members ``X`` and ``pred_stds`` (src/odometry.cpp:76-79, src/simpleMapMaker.cpp:119-122).
:class:`ICET` below keeps the same constructor arguments (same names, order, defaults and meaning) and
the same member names, and calls ``icet_solve`` in ``libicet_hip.so`` (include/icet_hip.h).

There is no CPU fallback: if the HIP library is missing or no GPU is usable this module raises.
"""
import contextlib
import ctypes as C
import os
import types
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ICET_HIP_LIB") or os.path.join(_HERE, "lib", "libicet_hip.so")   # override: kernel experiments only

ICET_OK, ICET_ERR_BAD_ARG, ICET_ERR_NO_DEVICE, ICET_ERR_HIP, ICET_ERR_NOMEM, ICET_ERR_UNSUPPORTED = range(6)
_STATUS_NAMES = {0: "ICET_OK", 1: "ICET_ERR_BAD_ARG", 2: "ICET_ERR_NO_DEVICE", 3: "ICET_ERR_HIP", 4: "ICET_ERR_NOMEM", 5: "ICET_ERR_UNSUPPORTED"}
FLAG_TIMING = 1
FLAG_TRUE_SORT = 2      # non-parity extension, see include/icet_hip.h
FLAG_REJECT_MOVING = 4  # non-parity extension (moving-object rejection of the Python variant), see include/icet_hip.h
FLAG_ROUNDTRIP_SCAN2 = 16  # parity-study option: the reference's two spherical round trips of scan 2 (see include/icet_hip.h)
FLAG_DOUBLE_W = 32         # accuracy option: per-voxel W in double instead of the reference's float COD (see include/icet_hip.h)
FLAG_HALF_GAP_BOUNDS = 8  # non-parity extension (half-gap cluster buffers of the Python variant; implies TRUE_SORT), see include/icet_hip.h

# every symbol include/icet_hip.h, include/icet_nodes.h and include/icet_io.h declare
EXPORTED_SYMBOLS = ("icet_create", "icet_destroy", "icet_last_error", "icet_version", "icet_solve", "icet_solve_begin", "icet_solve_keyframe_tables", "icet_solve_end", "icet_solve_batch",
                    "icet_solve_batch_device", "icet_sync", "icet_reserve", "icet_last_timing", "icet_last_timing_iters", "icet_keep_stats", "icet_debug_fetch", "icet_debug_gn_tail", "icet_debug_pinv3", "icet_debug_pinv3_double", "icet_debug_point_sums_device", "icet_debug_gn_terms_device", "icet_debug_fix", "icet_debug_spherical", "icet_set_option", "icet_keyframe_device", "icet_register_device", "icet_keyframe_device_n", "icet_register_device_n", "icet_register_indexed_device", "icet_solve_indexed", "icet_score_indexed_device", "icet_register_indexed_scored_device", "icet_solve_indexed_scored", "icet_score_indexed", "icet_select_best_device",
                    "icet_keyframe_store_create", "icet_keyframe_store_destroy", "icet_keyframe_store_last_error", "icet_keyframe_store_reserve", "icet_keyframe_store_put_device",
                    "icet_keyframe_store_register_device", "icet_keyframe_store_register_scored_device", "icet_keyframe_store_score_device", "icet_keyframe_store_debug_fetch",
                    "icet_keyframe_store_set_pose", "icet_keyframe_store_candidates_device", "icet_keyframe_store_close_device", "icet_pose_step_from_x",
                    "icet_keyframe_store_enable_appearance", "icet_keyframe_store_describe_device", "icet_keyframe_store_set_stamp",
                    "icet_keyframe_store_candidates_appearance_device", "icet_keyframe_store_close_appearance_device",
                    "icet_keyframe_store_enable_coarse", "icet_keyframe_store_coarse_grid_device", "icet_keyframe_store_coarse_align_device",
                    "icet_keyframe_store_close_coarse_device",
                    "icet_debug_block_tridiag", "icet_pose_graph_optimize", "icet_pose_graph_optimize_device", "icet_pose_graph_optimize_robust", "icet_pose_graph_optimize_robust_device", "icet_debug_pose_graph_step", "icet_debug_pose_graph_direct",
                    "icet_pose_graph_marginals", "icet_pose_graph_marginals_device", "icet_debug_pose_graph_marginals",
                    "icet_pose_graph_covariance_columns", "icet_pose_graph_covariance_columns_device", "icet_pose_graph_gate", "icet_pose_graph_gate_device",
                    "icet_voxel_map_create", "icet_voxel_map_destroy", "icet_voxel_map_last_error", "icet_voxel_map_clear", "icet_voxel_map_add_device",
                    "icet_voxel_map_add_posed_device", "icet_voxel_map_stats", "icet_voxel_map_extract_device", "icet_voxel_map_extract",
                    "icet_voxel_map_index", "icet_voxel_map_query_device", "icet_voxel_map_query_posed_device",
                    "icet_voxel_map_evidence_device", "icet_voxel_map_evidence_posed_device", "icet_voxel_map_evidence_fetch_device",
                    "icet_voxel_map_enable_shape", "icet_voxel_map_extract_shape_device", "icet_voxel_map_extract_shape",
                    "icet_voxel_map_register_device", "icet_voxel_map_register_posed_device", "icet_debug_voxel_map_register_terms",
                    "icet_voxel_map_save", "icet_voxel_map_load", "icet_voxel_map_snapshot_info", "icet_voxel_map_merge_device",
                    "icet_deskewer_create", "icet_deskewer_destroy", "icet_deskewer_last_error", "icet_deskew_device", "icet_deskew",
                    "icet_deskew_twists_from_poses_device", "icet_twist_from_pose", "icet_pose_from_twist", "icet_debug_deskew_rows",
                    "icet_keyframe_store_save", "icet_keyframe_store_load", "icet_keyframe_store_snapshot_info", "icet_keyframe_store_snapshot_slots",
                    "icet_multi_create", "icet_multi_destroy", "icet_multi_last_error", "icet_multi_devices", "icet_multi_context",
                    "icet_multi_solve_batch", "icet_multi_solve_batch_device", "icet_multi_solve_batch_device_after", "icet_multi_solve_batch_device_async", "icet_multi_sync", "icet_multi_set_option",
                    "icet_node_create", "icet_node_destroy", "icet_node_last_error", "icet_node_push", "icet_node_push_device", "icet_node_push_many_device", "icet_node_map",
                    "icet_node_prev_scan", "icet_node_aligned", "icet_node_snail_trail", "icet_node_last_timing", "icet_debug_node_tail", "icet_stream", "icet_device",
                    "icet_node_group_create", "icet_node_group_destroy", "icet_node_group_last_error", "icet_node_group_push_device", "icet_node_group_map",
                    "icet_node_group_prev_scan", "icet_node_group_aligned", "icet_node_group_snail_trail",
                    "icet_load_scan", "icet_free_scan", "icet_save_scan_npy")
_NON_STATUS = ("icet_version", "icet_last_error", "icet_node_last_error", "icet_node_group_last_error", "icet_stream", "icet_device", "icet_free_scan", "icet_multi_last_error", "icet_multi_devices", "icet_multi_context",
               "icet_keyframe_store_last_error", "icet_pose_step_from_x", "icet_voxel_map_last_error", "icet_deskewer_last_error")


class IcetError(RuntimeError):
    def __init__(self, status, msg=""):
        self.status = status
        super().__init__("%s%s" % (_STATUS_NAMES.get(status, str(status)), (": " + msg) if msg else ""))


class Params(C.Structure):
    _fields_ = [("runlen", C.c_int32), ("bins_phi", C.c_int32), ("bins_theta", C.c_int32), ("n", C.c_int32),
                ("thresh", C.c_float), ("buff", C.c_float), ("flags", C.c_int32)]


# icet_score (include/icet_hip.h): the registration score, 32 bytes
SCORE_DTYPE = np.dtype([("chi2", "<f4"), ("chi2_per_voxel", "<f4"), ("voxels", "<i4"), ("points_in", "<i4"), ("points", "<i4"), ("overlap", "<f4"),
                        ("reserved", "<i4", (2,))])
assert SCORE_DTYPE.itemsize == 32
# a voxel's raw accumulator record (icet_debug_point_sums_device): the counts and the nine 2^36 fixed-point sums of d = q - mu1, 80 bytes
POINT_SUMS_DTYPE = np.dtype([("n2", "<u4"), ("m", "<u4"), ("sums", "<i8", (9,))])
assert POINT_SUMS_DTYPE.itemsize == 80


class ClosureQuery(C.Structure):
    """icet_closure_query (include/icet_hip.h), 32 bytes."""
    _fields_ = [("radius", C.c_float), ("max_candidates", C.c_int32), ("min_stamp_gap", C.c_int64), ("n_starts", C.c_int32),
                ("max_chi2_per_voxel", C.c_float), ("min_voxels", C.c_int32), ("reserved", C.c_int32)]


class AppearanceParams(C.Structure):
    """icet_appearance_params (include/icet_hip.h), 32 bytes."""
    _fields_ = [("sectors", C.c_int32), ("rings", C.c_int32), ("rho_max", C.c_float), ("z_lo", C.c_float), ("z_hi", C.c_float), ("reserved", C.c_int32 * 3)]


class CoarseParams(C.Structure):
    """icet_coarse_params (include/icet_hip.h), 32 bytes."""
    _fields_ = [("cells", C.c_int32), ("cell", C.c_float), ("z_lo", C.c_float), ("z_hi", C.c_float), ("min_span", C.c_float), ("reserved", C.c_int32 * 3)]


class MapParams(C.Structure):
    """icet_voxel_map_params (include/icet_hip.h), 32 bytes."""
    _fields_ = [("cell", C.c_float), ("min_range", C.c_float), ("max_range", C.c_float), ("table_log2", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


class MapStats(C.Structure):
    """struct icet_voxel_map_stats (include/icet_hip.h), 64 bytes."""
    _fields_ = [("points_in", C.c_int64), ("points_kept", C.c_int64), ("points_nonfinite", C.c_int64), ("points_outside", C.c_int64), ("points_dropped", C.c_int64),
                ("cells_occupied", C.c_int32), ("cells_out", C.c_int32), ("cells_negative", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32 * 2)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_[:9]}


VOXEL_MAP_OK, VOXEL_MAP_TABLE_FULL, VOXEL_MAP_NEGATIVE, VOXEL_MAP_TRUNCATED = 0, 1, 2, 4
VOXEL_MAP_QUERY_BAD_POSE = 8      # status bit of a query
VOXEL_MAP_QUERY_WORLD = 1         # flag of a query
VOXEL_MAP_QUERY_STATIC = 2        # flag of a query: the cells the current evidence calls transient take no part
VOXEL_MAP_MAX_QUERIES = 256
MAP_QUERY_CHUNK = 2048            # ICET_VOXEL_MAP_QUERY_CHUNK: index entries per block of a query (the sizes at which its kernels take another path)


class MapQuery(C.Structure):
    """icet_voxel_map_query (include/icet_hip.h), 32 bytes."""
    _fields_ = [("min_range", C.c_float), ("max_range", C.c_float), ("min_points", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]


class MapEvidence(C.Structure):
    """icet_voxel_map_evidence (include/icet_hip.h), 32 bytes."""
    _fields_ = [("min_range", C.c_float), ("max_range", C.c_float), ("margin", C.c_float), ("image_log2", C.c_int32), ("window", C.c_int32), ("min_miss", C.c_int32),
                ("agree_factor", C.c_int32), ("flags", C.c_int32)]


class MapEvidenceStats(C.Structure):
    """struct icet_voxel_map_evidence_stats (include/icet_hip.h), 32 bytes."""
    _fields_ = [("rows_imaged", C.c_int64), ("cells", C.c_int32), ("cells_transient", C.c_int32), ("scans_used", C.c_int32), ("scans_bad_pose", C.c_int32),
                ("reserved", C.c_int32 * 2)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_[:5]}


class MapSubmap(C.Structure):
    """icet_voxel_map_submap (include/icet_hip.h), 40 bytes: a host descriptor of device memory."""
    _fields_ = [("xyz", C.c_void_p), ("ld", C.c_int64), ("cap_rows", C.c_int64), ("count", C.c_void_p), ("key", C.c_void_p)]


class MapShape(C.Structure):
    """icet_voxel_map_shape (include/icet_hip.h), 48 bytes: the shape columns of an extract_shape call, each column-major over ld; a pointer left out is None."""
    _fields_ = [("cov", C.c_void_p), ("normal", C.c_void_p), ("evals", C.c_void_p), ("moments", C.c_void_p), ("ld", C.c_int64), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


VOXEL_MAP_REG_CONVERGED, VOXEL_MAP_REG_ITERATION_CAP, VOXEL_MAP_REG_STALLED, VOXEL_MAP_REG_NO_OVERLAP, VOXEL_MAP_REG_BAD_POSE = 0, 1, 2, 3, 4
VOXEL_MAP_REG_MAX_ITERS = 64
VOXEL_MAP_REG_NEIGHBOURS_7, VOXEL_MAP_REG_NEIGHBOURS_27 = 2, 4      # MapRegisterParams.flags: score a row against the best of 7 or 27 cells (0: its own cell)
VOXEL_MAP_REG_CHUNK = 2048        # rows per block of the row pass (the sizes at which it takes another path)


class MapRegisterParams(C.Structure):
    """icet_voxel_map_register_params (include/icet_hip.h), 72 bytes."""
    _fields_ = [("min_range", C.c_float), ("max_range", C.c_float), ("sigma_min", C.c_double), ("scale", C.c_double), ("tol_t", C.c_double), ("tol_r", C.c_double),
                ("lambda0", C.c_double), ("min_points", C.c_int32), ("min_matched", C.c_int32), ("max_iters", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class MapRegistration(C.Structure):
    """icet_voxel_map_registration (include/icet_hip.h), 328 bytes: the record of one query."""
    _fields_ = [("pose", C.c_float * 16), ("info", C.c_double * 21), ("g", C.c_double * 6), ("cost", C.c_double), ("cost_start", C.c_double), ("lambda_", C.c_double),
                ("rows_scored", C.c_int32), ("rows_matched", C.c_int32), ("iterations", C.c_int32), ("accepted", C.c_int32), ("status", C.c_int32),
                ("reserved", C.c_int32)]


MAP_REGISTRATION_DTYPE = np.dtype([("pose", "<f4", (16,)), ("info", "<f8", (21,)), ("g", "<f8", (6,)), ("cost", "<f8"), ("cost_start", "<f8"), ("lambda", "<f8"),
                                   ("rows_scored", "<i4"), ("rows_matched", "<i4"), ("iterations", "<i4"), ("accepted", "<i4"), ("status", "<i4"), ("reserved", "<i4")])
assert MAP_REGISTRATION_DTYPE.itemsize == 328 == C.sizeof(MapRegistration)
# one row of icet_debug_voxel_map_register_terms, 256 bytes
MAP_REGISTER_TERM_DTYPE = np.dtype([("key", "<u8"), ("cls", "<i4"), ("matched", "<i4"), ("s", "<f8"), ("omega", "<f8"), ("rho", "<f8"), ("g", "<f8", (6,)),
                                    ("H", "<f8", (21,))])
assert MAP_REGISTER_TERM_DTYPE.itemsize == 256
MAP_REGISTER_DEFAULTS = dict(min_range=0.0, max_range=0.0, sigma_min=0.02, scale=11.3449, tol_t=1e-4, tol_r=1e-5, lambda0=1e-3, min_points=5, min_matched=50,
                             max_iters=20)


def map_register_params(**kw):
    """A MapRegisterParams from keywords over MAP_REGISTER_DEFAULTS (the values a NULL params gives).  ``neighbours`` = 1 (default), 7 or 27: the cells a row is
    scored against the best of, as the bit of ``flags`` that names them (``flags=`` itself still passes through; both: the bits are joined)."""
    d = dict(MAP_REGISTER_DEFAULTS)
    extra = set(kw) - set(d) - {"flags", "neighbours"}
    if extra:
        raise TypeError("unknown registration parameter(s): " + ", ".join(sorted(extra)))
    d.update(kw)
    nb = d.pop("neighbours", 1)
    if nb not in (1, 7, 27) or isinstance(nb, bool):
        raise ValueError("neighbours must be 1, 7 or 27")
    d["flags"] = int(d.get("flags", 0)) | {1: 0, 7: VOXEL_MAP_REG_NEIGHBOURS_7, 27: VOXEL_MAP_REG_NEIGHBOURS_27}[nb]
    return MapRegisterParams(float(d["min_range"]), float(d["max_range"]), float(d["sigma_min"]), float(d["scale"]), float(d["tol_t"]), float(d["tol_r"]),
                             float(d["lambda0"]), int(d["min_points"]), int(d["min_matched"]), int(d["max_iters"]), int(d.get("flags", 0)))


def info_matrix(info21):
    """The symmetric 6 x 6 matrix of a record's 21 upper-triangle words (by rows)."""
    H = np.zeros((6, 6), np.float64)
    H[np.triu_indices(6)] = np.asarray(info21, np.float64).reshape(21)
    return H + np.triu(H, 1).T


def registration_cov(rec):
    """H^-1 of a registration record (a dict of VoxelMap.register, or anything with an ``info`` of 21 words): the 6 x 6 covariance of the pose in the record's
    tangent (translation, then rotation, world-aligned at the sensor origin).  NaN everywhere where H is not positive definite."""
    H = info_matrix(rec["info"])
    try:
        if not np.isfinite(H).all():
            raise np.linalg.LinAlgError("not finite")
        L = np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return np.full((6, 6), np.nan)
    Li = np.linalg.inv(L)
    return Li.T @ Li


def info_body_from_world(info, R):
    """A record's information in the pose graph's right-hand (body) tangent: both 3-blocks rotated by the pose's rotation R, A = diag(R, R), A^T H A.  ``info``:
    21 words or a 6 x 6 matrix; returns 6 x 6."""
    H = np.asarray(info, np.float64)
    H = info_matrix(H) if H.size == 21 else H.reshape(6, 6)
    R = np.asarray(R, np.float64).reshape(3, 3)
    A = np.zeros((6, 6)); A[:3, :3] = R; A[3:, 3:] = R
    return A.T @ H @ A


def cov_matrix(cov6):
    """The symmetric 3 x 3 matrices of (..., 6) covariance rows in extract_shape's order xx, xy, xz, yy, yz, zz: an (..., 3, 3) array of the same dtype."""
    c = np.asarray(cov6)
    return c[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(c.shape[:-1] + (3, 3))


def shape_features(evals):
    """Linearity (l2 - l1) / l2, planarity (l1 - l0) / l2 and sphericity l0 / l2 from (..., 3) ASCENDING eigenvalues l0 <= l1 <= l2, as extract_shape writes
    them: a dict of float64 arrays.  A cell whose largest eigenvalue is not positive (one row, or coincident rows) gives zeros."""
    e = np.asarray(evals, np.float64)
    l0, l1, l2 = e[..., 0], e[..., 1], e[..., 2]
    ok = l2 > 0
    den = np.where(ok, l2, 1.0)
    return dict(linearity=np.where(ok, (l2 - l1) / den, 0.0), planarity=np.where(ok, (l1 - l0) / den, 0.0), sphericity=np.where(ok, l0 / den, 0.0))


DESKEW_TIME_ARRAY, DESKEW_TIME_COLUMN_FAST, DESKEW_TIME_COLUMN_SLOW = 0, 1, 2      # ICET_DESKEW_TIME_*


class DeskewScan(C.Structure):
    """icet_deskew_scan (include/icet_hip.h), 128 bytes: one scan of a deskew call, its times and the motion of its sweep."""
    _fields_ = [("src", C.c_void_p), ("n", C.c_int64), ("ld", C.c_int64), ("dst", C.c_void_p), ("ld_out", C.c_int64), ("time", C.c_void_p),
                ("time_mode", C.c_int32), ("period", C.c_int32), ("t0", C.c_double), ("inv_span", C.c_double), ("s_ref", C.c_double), ("twist", C.c_double * 6)]


class DeskewCounts(C.Structure):
    """icet_deskew_counts (include/icet_hip.h), 64 bytes: the rows of one scan by class."""
    _fields_ = [("moved", C.c_int64), ("zero", C.c_int64), ("nonfinite", C.c_int64), ("bad_time", C.c_int64), ("out_of_range", C.c_int64), ("reserved", C.c_int64 * 3)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_[:5]}


def deskew_scan(src, n, ld, dst=None, ld_out=None, time=None, time_mode=DESKEW_TIME_ARRAY, period=0, t0=0.0, span=1.0, ref=1.0, twist=(0, 0, 0, 0, 0, 0)):
    """A DeskewScan from addresses (device or host, as the call takes them): dst None is in place; span is the time of a whole sweep (the record carries its
    reciprocal, taken here once); ref the sweep fraction whose frame the rows are carried into (0 sweep start, 1 sweep end)."""
    tw = np.asarray(twist, np.float64).reshape(6)
    return DeskewScan(int(src) if src else None, int(n), int(ld), int(dst if dst is not None else src) if (dst if dst is not None else src) else None,
                      int(ld if ld_out is None else ld_out), int(time) if time else None, int(time_mode), int(period), float(t0), 1.0 / float(span), float(ref),
                      (C.c_double * 6)(*[float(v) for v in tw]))


def voxel_key_cells(key):
    """The integer cell indices (c_x, c_y, c_z) of voxel-map keys (include/icet_hip.h, the rule's step 5): an (..., 3) int64 array."""
    k = np.asarray(key, np.uint64)
    m = np.uint64(0x1FFFFF)
    return np.stack([((k >> np.uint64(42)) & m).astype(np.int64), ((k >> np.uint64(21)) & m).astype(np.int64), (k & m).astype(np.int64)], axis=-1) - (1 << 20)


class SnapshotInfo(C.Structure):
    """icet_snapshot_info (include/icet_hip.h), 120 bytes: what a snapshot file of a keyframe store says about itself."""
    _fields_ = [("shape", Params), ("V", C.c_int32), ("entries", C.c_int32), ("highest_slot", C.c_int32), ("has_appearance", C.c_int32), ("has_coarse", C.c_int32),
                ("appearance", AppearanceParams), ("coarse", CoarseParams), ("file_bytes", C.c_int64)]


class MapSnapshotInfo(C.Structure):
    """struct icet_voxel_map_snapshot_info (include/icet_hip.h), 96 bytes: what a snapshot file of a voxel map says about itself."""
    _fields_ = [("cell", C.c_float), ("min_range", C.c_float), ("max_range", C.c_float), ("shaped", C.c_int32), ("words_per_entry", C.c_int32), ("reserved0", C.c_int32),
                ("entries", C.c_int64), ("points_in", C.c_int64), ("points_kept", C.c_int64), ("points_nonfinite", C.c_int64), ("points_outside", C.c_int64),
                ("points_dropped", C.c_int64), ("file_bytes", C.c_int64), ("payload_checksum", C.c_uint64), ("reserved", C.c_int32 * 2)]


class CoarseSearch(C.Structure):
    """icet_coarse_search (include/icet_hip.h), 32 bytes."""
    _fields_ = [("window", C.c_int32), ("n_yaw", C.c_int32), ("yaw_step", C.c_float), ("half_turn", C.c_int32), ("min_score", C.c_int32), ("reserved", C.c_int32 * 3)]


class CoarseMatch(C.Structure):
    """icet_coarse_match (include/icet_hip.h), 32 bytes."""
    _fields_ = [("score", C.c_int32), ("a", C.c_int32), ("b", C.c_int32), ("h", C.c_int32), ("live_bits", C.c_int32), ("key_bits", C.c_int32), ("found", C.c_int32),
                ("reserved", C.c_int32)]


# icet_coarse_match as a NumPy dtype (a device buffer of records comes back as bytes)
COARSE_MATCH_DTYPE = np.dtype([("score", "<i4"), ("a", "<i4"), ("b", "<i4"), ("h", "<i4"), ("live_bits", "<i4"), ("key_bits", "<i4"), ("found", "<i4"), ("reserved", "<i4")])
assert COARSE_MATCH_DTYPE.itemsize == 32 == C.sizeof(CoarseMatch) == C.sizeof(CoarseSearch) == C.sizeof(CoarseParams) and C.sizeof(SnapshotInfo) == 120


class Score(C.Structure):
    """icet_score (include/icet_hip.h), 32 bytes."""
    _fields_ = [("chi2", C.c_float), ("chi2_per_voxel", C.c_float), ("voxels", C.c_int32), ("points_in", C.c_int32), ("points", C.c_int32),
                ("overlap", C.c_float), ("reserved", C.c_int32 * 2)]


class Closure(C.Structure):
    """icet_closure (include/icet_hip.h), 288 bytes: one record per query of icet_keyframe_store_close_device."""
    _fields_ = [("slot", C.c_int32), ("reg", C.c_int32), ("accepted", C.c_int32), ("n_candidates", C.c_int32), ("stamp", C.c_int64), ("d2", C.c_float),
                ("reserved0", C.c_int32), ("x0", C.c_float * 6), ("reserved1", C.c_int32 * 2), ("out", C.c_float * 48), ("score", Score)]


# the same record as a NumPy dtype (a device buffer of records comes back as bytes)
CLOSURE_DTYPE = np.dtype([("slot", "<i4"), ("reg", "<i4"), ("accepted", "<i4"), ("n_candidates", "<i4"), ("stamp", "<i8"), ("d2", "<f4"), ("reserved0", "<i4"),
                          ("x0", "<f4", (6,)), ("reserved1", "<i4", (2,)), ("out", "<f4", (48,)), ("score", SCORE_DTYPE)])
assert CLOSURE_DTYPE.itemsize == 288 == C.sizeof(Closure) and C.sizeof(ClosureQuery) == 32 and C.sizeof(Score) == 32 and C.sizeof(AppearanceParams) == 32


class PoseGraphOptions(C.Structure):
    """icet_pose_graph_options (include/icet_hip.h), 32 bytes."""
    _fields_ = [("gn_iters", C.c_int32), ("max_pcg", C.c_int32), ("dx_tol", C.c_double), ("damping", C.c_double), ("pcg_tol", C.c_double)]


class PoseGraphResult(C.Structure):
    """icet_pose_graph_result (include/icet_hip.h), 40 bytes."""
    _fields_ = [("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("max_dx", C.c_double), ("status", C.c_int32), ("gn_iterations", C.c_int32),
                ("pcg_iterations", C.c_int32), ("solver", C.c_int32)]


class PoseGraphRobust(C.Structure):
    """icet_pose_graph_robust (include/icet_hip.h), 16 bytes."""
    _fields_ = [("kind", C.c_int32), ("flags", C.c_int32), ("scale", C.c_double)]


class PoseGraphRobustResult(C.Structure):
    """icet_pose_graph_robust_result (include/icet_hip.h), 64 bytes."""
    _fields_ = [("base", PoseGraphResult), ("cost_initial", C.c_double), ("cost_final", C.c_double), ("downweighted", C.c_int32), ("reserved", C.c_int32)]


class PoseGraphStep(C.Structure):
    """icet_pose_graph_step (include/icet_hip.h), 152 bytes."""
    ARRAYS = ("J", "res", "chi_start", "chi_trial", "D", "B", "A", "g", "x", "Pt", "q", "cg_scalars")
    _fields_ = [(k, C.c_void_p) for k in ARRAYS] + [(k, C.c_int32) for k in ("cg_capacity", "factor_status", "cg_status", "band_solves", "cg_end", "cap", "c_offband", "trial")] + \
               [(k, C.c_double) for k in ("chi2_start", "chi2_trial", "max_dx")]


class PoseGraphDirectStep(C.Structure):
    """icet_pose_graph_direct_step (include/icet_hip.h), 176 bytes."""
    ARRAYS = ("D", "B", "A", "g", "Z", "Wm", "L", "Ks", "Lk", "x0", "x", "Pt", "chi_trial", "q")
    _fields_ = [(k, C.c_void_p) for k in ARRAYS] + [("ends", C.c_void_p)] + \
               [(k, C.c_int32) for k in ("ends_capacity", "m", "factor_status", "wm_status", "ks_status", "band_solves", "trial", "reserved")] + \
               [(k, C.c_double) for k in ("chi2_start", "chi2_trial", "max_dx")]


class PoseGraphMarginalsResult(C.Structure):
    """icet_pose_graph_marginals_result (include/icet_hip.h), 24 bytes."""
    _fields_ = [(k, C.c_int32) for k in ("status", "m", "factor_status", "wm_status", "ks_status", "reserved")]


class PoseGraphMarginalsDebug(C.Structure):
    """icet_pose_graph_marginals_debug (include/icet_hip.h), 80 bytes."""
    ARRAYS = ("D", "B", "A", "band_cov", "cov")
    _fields_ = [(k, C.c_void_p) for k in ARRAYS] + [("ends", C.c_void_p), ("ends_capacity", C.c_int32), ("reserved", C.c_int32), ("result", PoseGraphMarginalsResult)]


class PoseGraphGateResult(C.Structure):
    """icet_pose_graph_gate_result (include/icet_hip.h), 32 bytes."""
    _fields_ = [("marg", PoseGraphMarginalsResult), ("n_targets", C.c_int32), ("rejected", C.c_int32)]


assert C.sizeof(PoseGraphGateResult) == 32
assert C.sizeof(PoseGraphOptions) == 32 and C.sizeof(PoseGraphResult) == 40 and C.sizeof(PoseGraphStep) == 152 and C.sizeof(PoseGraphDirectStep) == 176
assert C.sizeof(PoseGraphMarginalsResult) == 24 and C.sizeof(PoseGraphMarginalsDebug) == 80
assert C.sizeof(PoseGraphRobust) == 16 and C.sizeof(PoseGraphRobustResult) == 64
# icet_pose_graph_robust: the kinds by name, flag bit 0, the default threshold (the 99 % quantile of chi2 with six degrees of freedom)
PG_ROBUST_KINDS = {"huber": 1, "cauchy": 2, "geman_mcclure": 3}
PG_ROBUST_ODOMETRY = 1
PG_ROBUST_DEFAULT_SCALE = 16.8119
# option "pg_solver": the pose-graph optimiser's linear solve
PG_SOLVER_CG, PG_SOLVER_DIRECT, PG_SOLVER_AUTO = range(3)
PG_SOLVERS = {"cg": PG_SOLVER_CG, "direct": PG_SOLVER_DIRECT, "auto": PG_SOLVER_AUTO}
PG_DIRECT_MAX_ENDS = 128
PG_MAX_TARGETS = 32          # icet_pose_graph_covariance_columns: targets per call; icet_pose_graph_gate: distinct live nodes per call
PG_GATE_MAX_CANDIDATES = 512


def pose_graph_ends(n, closures, fixed=None):
    """The END nodes of the direct solve, ascending: the distinct ends of the closures that lie off the band (|i - j| >= 2) between two free nodes (node 0 and
    the nodes with fixed[k] != 0 are not free)."""
    fx = np.zeros(n, bool); fx[0] = True
    if fixed is not None:
        fx |= np.asarray(fixed).reshape(-1) != 0
    ends = set()
    for c in closures:
        i, j = int(c[0]), int(c[1])
        if abs(i - j) >= 2 and not fx[i] and not fx[j]:
            ends.update((i, j))
    return sorted(ends)
# icet_pose_graph_step.cg_end
PG_CG_TOLERANCE, PG_CG_ZERO, PG_CG_CAP, PG_CG_FAILED = range(4)
# icet_pose_graph_result.status
POSE_GRAPH_CONVERGED, POSE_GRAPH_ITERATION_CAP, POSE_GRAPH_NOT_POSITIVE_DEFINITE, POSE_GRAPH_NON_FINITE, POSE_GRAPH_STALLED = range(5)


def _closure_weights(closures, weights, n):
    closures = list(closures)
    w = np.asarray(weights, np.float64).reshape(-1)
    if n is None and w.shape[0] == len(closures):
        return closures, w
    if n is not None and w.shape[0] == int(n) - 1 + len(closures):
        return closures, w[int(n) - 1:]
    raise IcetError(ICET_ERR_BAD_ARG, "weights must hold one entry per closure, or with n the n - 1 + C entries of a result's edge_weight")


def reweighted_closures(closures, weights, n=None):
    """``closures`` ((i, j, X, info) tuples) with every information matrix scaled by its closure's final weight.  ``weights`` is one entry per closure; or,
    with ``n`` the number of poses, the ``edge_weight`` of a robust optimize_pose_graph (n - 1 + C entries: the closures' are the last).  Any other length is
    refused.  Context.pose_graph_marginals on the result gives the covariances at the robust optimum: H there is sum w_e J^T Omega J."""
    closures, w = _closure_weights(closures, weights, n)
    return [(c[0], c[1], c[2], (np.asarray(c[3], np.float64) * wi).astype(np.float32)) for c, wi in zip(closures, w)]


def inlier_closures(closures, weights, min_weight=0.5, n=None):
    """The closures whose final weight is at least ``min_weight`` (``weights`` and ``n`` as in reweighted_closures): what a robust run kept."""
    closures, w = _closure_weights(closures, weights, n)
    return [c for c, wi in zip(closures, w) if wi >= min_weight]


def pose_stds(cov):
    """n x 6: the standard deviations of every pose from its marginal covariance ``cov`` (n x 6 x 6, Context.pose_graph_marginals): metres along the node's own
    axes, then radians of the rotation vector."""
    c = np.asarray(cov, np.float64).reshape(-1, 6, 6)
    return np.sqrt(np.einsum("kaa->ka", c))


def position_cov_world(poses, cov):
    """n x 3 x 3: the translation block of every pose's marginal covariance in the MAP frame, R_k Sigma_rho,rho R_k^T (the tangent of the right update moves a
    pose's position by R_k rho)."""
    R = np.asarray(poses, np.float64).reshape(-1, 4, 4)[:, :3, :3]
    c = np.asarray(cov, np.float64).reshape(-1, 6, 6)[:, :3, :3]
    return R @ c @ R.transpose(0, 2, 1)


def relative_cov(J, cov_i, cov_j, cov_ij):
    """6 x 6: J [[cov_i, cov_ij], [cov_ij^T, cov_j]] J^T for a 6 x 12 Jacobian J = [J_i | J_j] of a function of two poses -- the covariance of that function
    under the graph.  cov_i, cov_j are the poses' marginals (Context.pose_graph_marginals), cov_ij is block (i, j) of H^-1: ``cols[t][i]`` of
    Context.pose_graph_covariance_columns with targets[t] = j.  For callers with their own Jacobians; Context.pose_graph_gate has the optimiser's.  The result
    is symmetric bit for bit."""
    J = np.asarray(J, np.float64).reshape(6, 12)
    ci, cj, cij = (np.asarray(x, np.float64).reshape(6, 6) for x in (cov_i, cov_j, cov_ij))
    S = J @ np.block([[ci, cij], [cij.T, cj]]) @ J.T
    return 0.5 * (S + S.T)


def info_from_cov(cov):
    """The information matrix of a registration for the pose graph: the symmetrised pseudo-inverse of its 6 x 6 ``cov`` in double, rounded to float32."""
    c = np.asarray(cov, np.float64).reshape(6, 6)
    p = np.linalg.pinv(0.5 * (c + c.T), hermitian=True)
    return (0.5 * (p + p.T)).astype(np.float32)


def closure_edges(records, live_nodes, node_of_slot):
    """The closure edges (i, j, X, info) of the ACCEPTED records of find_closures, find_closures_by_appearance or find_closures_coarse: record q is the
    registration of live scan ``live_nodes[q]`` (node j) against the keyframe in its ``slot`` (node i = ``node_of_slot[slot]``, a dict or a sequence).  A
    record whose two ends are the same node is left out."""
    edges = []
    for q, r in enumerate(records):
        if r["slot"] is None or not r["accepted"]:
            continue
        i, j = int(node_of_slot[r["slot"]]), int(live_nodes[q])
        if i != j:
            edges.append((i, j, np.asarray(r["X"], np.float32).copy(), info_from_cov(r["cov"])))
    return edges


def closure_candidates(records, live_nodes, node_of_slot):
    """closure_edges with the record's covariance in the place of the information: the candidates (i, j, X, cov) of the ACCEPTED records, as
    Context.pose_graph_gate takes them.  find -> gate -> edges:
        cands = closure_candidates(records, live_nodes, node_of_slot)
        keep = ctx.pose_graph_gate(poses, odo_X, odo_info, closures, cands)["accepted"]
        closures += [(i, j, X, info_from_cov(cov)) for (i, j, X, cov), ok in zip(cands, keep) if ok]"""
    cands = []
    for q, r in enumerate(records):
        if r["slot"] is None or not r["accepted"]:
            continue
        i, j = int(node_of_slot[r["slot"]]), int(live_nodes[q])
        if i != j:
            cands.append((i, j, np.asarray(r["X"], np.float32).copy(), np.asarray(r["cov"], np.float32).reshape(6, 6).copy()))
    return cands


# The recommended start offsets of a query by appearance (INTEGRATION "Loop closure without poses"): the search gives the yaw, not the translation, so
# the starts are a 3 x 3 lattice of {-0.3, 0, 0.3} m in x and y around X0 = (0, 0, 0, 0, 0, yaw).
LATTICE_STARTS = np.array([[dx, dy, 0, 0, 0, 0] for dx in (-0.3, 0.0, 0.3) for dy in (-0.3, 0.0, 0.3)], np.float32)


def pose_step_from_X(X):
    """One step of a pose chain from a registration result X (icet_pose_step_from_x): the 4 x 4 float32 T = [R(X)^T | R(X)^T X_t]; a caller chains
    T_world,k = T_world,k-1 @ T.  This is the PHYSICAL sensor motion, not the chain icet_node_result.pose keeps (include/icet_hip.h, POSE)."""
    x = np.ascontiguousarray(np.asarray(X, np.float32).reshape(6))
    T = np.zeros(16, np.float32)
    load_library().icet_pose_step_from_x(x.ctypes.data, T.ctypes.data)
    return T.reshape(4, 4)


def twist_from_pose(T):
    """log of a 4 x 4 pose (icet_twist_from_pose): the twist (rho, phi) as six float64, exp of which is T.  Rotation angles below 3 rad."""
    t = np.ascontiguousarray(np.asarray(T, np.float64).reshape(16))
    xi = np.zeros(6, np.float64)
    st = load_library().icet_twist_from_pose(t.ctypes.data, xi.ctypes.data)
    if st != ICET_OK:
        raise IcetError(st, "icet_twist_from_pose")
    return xi


def pose_from_twist(xi, s=1.0):
    """exp(s xi) (icet_pose_from_twist): the 4 x 4 float64 pose of the sensor at sweep fraction s, in the sensor frame at s = 0."""
    x = np.ascontiguousarray(np.asarray(xi, np.float64).reshape(6))
    T = np.zeros(16, np.float64)
    st = load_library().icet_pose_from_twist(x.ctypes.data, float(s), T.ctypes.data)
    if st != ICET_OK:
        raise IcetError(st, "icet_pose_from_twist")
    return T.reshape(4, 4)


def twist_from_X(X):
    """The twist of one frame period under constant velocity, from a registration result X: twist_from_pose(pose_step_from_X(X))."""
    return twist_from_pose(pose_step_from_X(X))


def debug_deskew_rows(rows, twist, time=None, time_mode=DESKEW_TIME_ARRAY, period=0, t0=0.0, inv_span=1.0, ref=1.0):
    """The library's compiled body of the deskew rule on host rows (icet_debug_deskew_rows; no GPU): (N x 3 float32 rows out, int32 classes)."""
    p = np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, 3).T)
    n = p.shape[1]
    out = np.zeros_like(p); cls = np.zeros(max(n, 1), np.int32)
    tm = None if time is None else np.ascontiguousarray(np.asarray(time, np.float32).reshape(-1))
    m = DeskewScan(None, n, n, None, n, None, int(time_mode), int(period), float(t0), float(inv_span), float(ref), (C.c_double * 6)(*[float(v) for v in np.asarray(twist, np.float64).reshape(6)]))
    st = load_library().icet_debug_deskew_rows(C.byref(m), n, p[0].ctypes.data, p[1].ctypes.data, p[2].ctypes.data, _data(tm), out[0].ctypes.data, out[1].ctypes.data,
                                               out[2].ctypes.data, cls.ctypes.data)
    if st != ICET_OK:
        raise IcetError(st, "icet_debug_deskew_rows")
    return np.ascontiguousarray(out.T), cls[:n].copy()


def scores_as_dict(rec):
    """An icet_score array (SCORE_DTYPE) as named arrays: chi2, chi2_per_voxel, voxels, points_in, points, overlap."""
    return {k: np.array(rec[k]) for k in ("chi2", "chi2_per_voxel", "voxels", "points_in", "points", "overlap")}


class NodeParams(C.Structure):
    """icet_node_params (include/icet_nodes.h)."""
    _fields_ = [("solve", Params), ("min_range", C.c_float), ("seed_x0", C.c_int32), ("trans_thresh", C.c_float), ("rot_thresh", C.c_float),
                ("map_capacity", C.c_int32), ("map_downsample", C.c_int32), ("flags", C.c_int32)]


class NodeResult(C.Structure):
    _fields_ = [("solved", C.c_int32), ("diverged", C.c_int32), ("n_kept", C.c_int64), ("X", C.c_float * 6), ("pred_stds", C.c_float * 6),
                ("pose", C.c_float * 16), ("quat", C.c_float * 4), ("map_rows", C.c_int64)]


class DevScan(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("n", C.c_int64), ("ld", C.c_int64)]


_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)


class Aux(C.Structure):
    _fields_ = [("cluster_bounds", _F), ("n1_raw", _I), ("has_fit", _I), ("mu1", _F), ("sigma1", _F), ("evecs1", _F), ("l_diag", _F),
                ("x_hist", _F), ("htwh", _F), ("htwdz", _F), ("n2_raw", _I), ("n2_in", _I), ("test_points", _F), ("points2", _F),
                ("points1_spherical", _F), ("point_index1", _I), ("bin_start1", _I), ("points2_spherical", _F), ("voxel2", _I), ("cond_info", _F)]


_lib = None


def load_library():
    """dlopen libicet_hip.so (built in-tree by ``__graft_entry__.build()`` / ``make -C icet_amd/csrc``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IcetError(ICET_ERR_HIP, "HIP library not built: %s is missing (run `make -C icet_amd/csrc`); "
                                      "there is no CPU fallback for this path" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.icet_version.restype = C.c_char_p
    L.icet_last_error.restype = C.c_char_p
    L.icet_last_error.argtypes = [C.c_void_p]
    L.icet_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p]
    L.icet_destroy.argtypes = [C.c_void_p]
    L.icet_sync.argtypes = [C.c_void_p]
    L.icet_reserve.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.c_int64, C.c_int64]
    L.icet_solve.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Aux)]
    L.icet_solve_begin.argtypes = L.icet_solve.argtypes
    L.icet_solve_end.argtypes = [C.c_void_p]
    L.icet_solve_keyframe_tables.argtypes = [C.c_void_p]
    L.icet_solve_batch.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.icet_solve_batch_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.POINTER(DevScan), C.POINTER(DevScan), C.c_void_p, C.c_void_p]
    L.icet_last_timing.argtypes = [C.c_void_p, C.c_void_p]
    L.icet_last_timing_iters.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    L.icet_keep_stats.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.icet_debug_fetch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
    L.icet_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
    L.icet_debug_gn_tail.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.icet_debug_pinv3.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.icet_debug_pinv3_double.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.icet_debug_point_sums_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.c_void_p, C.POINTER(DevScan), C.c_void_p, C.c_void_p]
    L.icet_debug_gn_terms_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.c_void_p, C.POINTER(DevScan), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.icet_debug_fix.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.icet_debug_spherical.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    L.icet_keyframe_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.POINTER(DevScan)]
    L.icet_register_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.POINTER(DevScan), C.c_void_p, C.c_void_p]
    L.icet_keyframe_device_n.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.POINTER(DevScan), C.c_void_p]
    L.icet_register_device_n.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.POINTER(DevScan), C.c_void_p, C.c_void_p, C.c_void_p]
    L.icet_register_indexed_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.c_void_p, C.POINTER(DevScan), C.c_void_p, C.c_void_p]
    L.icet_solve_indexed.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.icet_score_indexed_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.c_void_p, C.POINTER(DevScan), C.c_void_p, C.c_void_p]
    L.icet_register_indexed_scored_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.c_void_p, C.POINTER(DevScan), C.c_void_p, C.c_void_p, C.c_void_p]
    L.icet_solve_indexed_scored.argtypes = L.icet_solve_indexed.argtypes + [C.c_void_p]
    L.icet_score_indexed.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.icet_select_best_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.icet_keyframe_store_create.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.POINTER(C.c_void_p)]
    L.icet_keyframe_store_destroy.argtypes = [C.c_void_p]
    L.icet_keyframe_store_last_error.argtypes = [C.c_void_p]; L.icet_keyframe_store_last_error.restype = C.c_char_p
    L.icet_keyframe_store_reserve.argtypes = [C.c_void_p, C.c_int32]
    L.icet_keyframe_store_put_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(DevScan), C.c_void_p]
    L.icet_keyframe_store_register_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.c_void_p, C.POINTER(DevScan), C.c_void_p, C.c_void_p]
    L.icet_keyframe_store_register_scored_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.c_void_p, C.POINTER(DevScan), C.c_void_p, C.c_void_p, C.c_void_p]
    L.icet_keyframe_store_score_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.c_void_p, C.POINTER(DevScan), C.c_void_p, C.c_void_p]
    L.icet_keyframe_store_debug_fetch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64]
    L.icet_keyframe_store_set_pose.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.icet_keyframe_store_candidates_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(ClosureQuery), C.c_void_p, C.c_void_p]
    L.icet_keyframe_store_close_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.POINTER(DevScan), C.c_void_p, C.c_void_p, C.POINTER(ClosureQuery), C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.icet_pose_step_from_x.argtypes = [C.c_void_p, C.c_void_p]; L.icet_pose_step_from_x.restype = None
    L.icet_debug_block_tridiag.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    L.icet_pose_graph_optimize.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(PoseGraphOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PoseGraphResult)]
    L.icet_pose_graph_optimize_device.argtypes = L.icet_pose_graph_optimize.argtypes
    L.icet_pose_graph_optimize_robust.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.POINTER(PoseGraphOptions), C.POINTER(PoseGraphRobust), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.POINTER(PoseGraphRobustResult)]
    L.icet_pose_graph_optimize_robust_device.argtypes = L.icet_pose_graph_optimize_robust.argtypes
    L.icet_debug_pose_graph_direct.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.POINTER(PoseGraphOptions), C.c_int32, C.c_void_p, C.POINTER(PoseGraphDirectStep)]
    L.icet_pose_graph_marginals.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.POINTER(PoseGraphMarginalsResult)]
    L.icet_pose_graph_marginals_device.argtypes = L.icet_pose_graph_marginals.argtypes
    L.icet_pose_graph_covariance_columns.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PoseGraphMarginalsResult)]
    L.icet_pose_graph_covariance_columns_device.argtypes = L.icet_pose_graph_covariance_columns.argtypes
    L.icet_pose_graph_gate.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(PoseGraphGateResult)]
    L.icet_pose_graph_gate_device.argtypes = L.icet_pose_graph_gate.argtypes
    L.icet_debug_pose_graph_marginals.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.POINTER(PoseGraphMarginalsDebug)]
    L.icet_debug_pose_graph_step.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(PoseGraphOptions), C.c_int32, C.c_void_p, C.POINTER(PoseGraphStep)]
    L.icet_keyframe_store_enable_appearance.argtypes = [C.c_void_p, C.POINTER(AppearanceParams)]
    L.icet_keyframe_store_describe_device.argtypes = [C.c_void_p, C.c_int32, C.POINTER(DevScan), C.c_void_p, C.c_void_p, C.c_void_p]
    L.icet_keyframe_store_set_stamp.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.icet_keyframe_store_candidates_appearance_device.argtypes = [C.c_void_p, C.c_int32, C.POINTER(DevScan), C.c_void_p, C.POINTER(ClosureQuery), C.c_void_p, C.c_void_p,
                                                                   C.c_void_p, C.c_void_p]
    L.icet_keyframe_store_close_appearance_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.POINTER(DevScan), C.c_void_p, C.POINTER(ClosureQuery), C.c_void_p,
                                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.icet_keyframe_store_enable_coarse.argtypes = [C.c_void_p, C.POINTER(CoarseParams)]
    L.icet_keyframe_store_coarse_grid_device.argtypes = [C.c_void_p, C.c_int32, C.POINTER(DevScan), C.c_void_p, C.c_void_p]
    L.icet_keyframe_store_coarse_align_device.argtypes = [C.c_void_p, C.c_int32, C.POINTER(DevScan), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(CoarseSearch),
                                                          C.c_void_p, C.c_void_p]
    L.icet_keyframe_store_close_coarse_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.POINTER(DevScan), C.c_void_p, C.c_void_p, C.POINTER(ClosureQuery),
                                                          C.POINTER(CoarseSearch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.icet_voxel_map_create.argtypes = [C.c_void_p, C.POINTER(MapParams), C.POINTER(C.c_void_p)]
    L.icet_voxel_map_destroy.argtypes = [C.c_void_p]
    L.icet_voxel_map_last_error.argtypes = [C.c_void_p]; L.icet_voxel_map_last_error.restype = C.c_char_p
    L.icet_voxel_map_clear.argtypes = [C.c_void_p]
    L.icet_voxel_map_add_device.argtypes = [C.c_void_p, C.c_int32, C.POINTER(DevScan), C.c_void_p, C.c_int32]
    L.icet_voxel_map_add_posed_device.argtypes = L.icet_voxel_map_add_device.argtypes
    L.icet_voxel_map_stats.argtypes = [C.c_void_p, C.c_int32, C.POINTER(MapStats)]
    L.icet_voxel_map_extract_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(MapStats)]
    L.icet_voxel_map_extract.argtypes = L.icet_voxel_map_extract_device.argtypes
    L.icet_voxel_map_index.argtypes = [C.c_void_p, C.POINTER(MapStats)]
    L.icet_voxel_map_query_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(MapQuery), C.POINTER(MapSubmap), C.c_void_p, C.c_void_p, C.c_void_p]
    L.icet_voxel_map_query_posed_device.argtypes = L.icet_voxel_map_query_device.argtypes
    L.icet_voxel_map_evidence_device.argtypes = [C.c_void_p, C.c_int32, C.POINTER(DevScan), C.c_void_p, C.POINTER(MapEvidence), C.POINTER(MapEvidenceStats)]
    L.icet_voxel_map_evidence_posed_device.argtypes = L.icet_voxel_map_evidence_device.argtypes
    L.icet_voxel_map_evidence_fetch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.icet_voxel_map_enable_shape.argtypes = [C.c_void_p]
    L.icet_voxel_map_extract_shape_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(MapShape), C.POINTER(MapStats)]
    L.icet_voxel_map_extract_shape.argtypes = L.icet_voxel_map_extract_shape_device.argtypes
    L.icet_voxel_map_register_device.argtypes = [C.c_void_p, C.c_int32, C.POINTER(DevScan), C.c_void_p, C.POINTER(MapRegisterParams), C.c_void_p]
    L.icet_voxel_map_register_posed_device.argtypes = L.icet_voxel_map_register_device.argtypes
    L.icet_debug_voxel_map_register_terms.argtypes = [C.c_void_p, C.POINTER(DevScan), C.c_void_p, C.POINTER(MapRegisterParams), C.c_void_p]
    L.icet_voxel_map_save.argtypes = [C.c_void_p, C.c_char_p]
    L.icet_voxel_map_load.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    L.icet_voxel_map_snapshot_info.argtypes = [C.c_char_p, C.POINTER(MapSnapshotInfo)]
    L.icet_voxel_map_merge_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    L.icet_deskewer_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.icet_deskewer_destroy.argtypes = [C.c_void_p]
    L.icet_deskewer_last_error.argtypes = [C.c_void_p]; L.icet_deskewer_last_error.restype = C.c_char_p
    L.icet_deskew_device.argtypes = [C.c_void_p, C.c_int32, C.POINTER(DeskewScan), C.c_void_p, C.c_void_p]
    L.icet_deskew.argtypes = [C.c_void_p, C.c_int32, C.POINTER(DeskewScan), C.c_void_p]
    L.icet_deskew_twists_from_poses_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_void_p]
    L.icet_twist_from_pose.argtypes = [C.c_void_p, C.c_void_p]
    L.icet_pose_from_twist.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
    L.icet_debug_deskew_rows.argtypes = [C.POINTER(DeskewScan), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.icet_keyframe_store_save.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p]
    L.icet_keyframe_store_load.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    L.icet_keyframe_store_snapshot_info.argtypes = [C.c_char_p, C.POINTER(SnapshotInfo)]
    L.icet_keyframe_store_snapshot_slots.argtypes = [C.c_char_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    L.icet_multi_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32]
    L.icet_multi_destroy.argtypes = [C.c_void_p]
    L.icet_multi_last_error.argtypes = [C.c_void_p]; L.icet_multi_last_error.restype = C.c_char_p
    L.icet_multi_devices.argtypes = [C.c_void_p]; L.icet_multi_devices.restype = C.c_int32
    L.icet_multi_context.argtypes = [C.c_void_p, C.c_int32]; L.icet_multi_context.restype = C.c_void_p
    L.icet_multi_solve_batch.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.icet_multi_solve_batch_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.POINTER(DevScan), C.POINTER(DevScan), C.c_void_p, C.c_void_p]
    L.icet_multi_solve_batch_device_after.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.POINTER(DevScan), C.POINTER(DevScan), C.c_void_p, C.c_void_p, C.c_void_p]
    L.icet_multi_solve_batch_device_async.argtypes = L.icet_multi_solve_batch_device_after.argtypes
    L.icet_multi_sync.argtypes = [C.c_void_p]
    L.icet_multi_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
    L.icet_node_create.argtypes = [C.c_void_p, C.POINTER(NodeParams), C.POINTER(C.c_void_p)]
    L.icet_node_destroy.argtypes = [C.c_void_p]
    L.icet_node_last_error.argtypes = [C.c_void_p]; L.icet_node_last_error.restype = C.c_char_p
    L.icet_node_push.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(NodeResult)]
    L.icet_node_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(NodeResult)]
    L.icet_node_push_many_device.argtypes = [C.c_void_p, C.POINTER(DevScan), C.c_int32, C.POINTER(NodeResult)]
    L.icet_node_map.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.icet_node_last_timing.argtypes = [C.c_void_p, C.c_void_p]
    L.icet_node_prev_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.icet_node_aligned.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.icet_node_snail_trail.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.icet_debug_node_tail.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.icet_node_group_create.argtypes = [C.c_void_p, C.POINTER(NodeParams), C.c_int32, C.POINTER(C.c_void_p)]
    L.icet_node_group_destroy.argtypes = [C.c_void_p]
    L.icet_node_group_last_error.argtypes = [C.c_void_p]; L.icet_node_group_last_error.restype = C.c_char_p
    L.icet_node_group_push_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(DevScan), C.POINTER(NodeResult)]
    for name in ("icet_node_group_map", "icet_node_group_prev_scan", "icet_node_group_aligned", "icet_node_group_snail_trail"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.icet_load_scan.argtypes = [C.c_char_p, C.c_int32, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int64)]
    L.icet_free_scan.argtypes = [C.POINTER(C.c_float)]; L.icet_free_scan.restype = None
    L.icet_save_scan_npy.argtypes = [C.c_char_p, C.c_void_p, C.c_int64, C.c_int64]
    L.icet_stream.argtypes = [C.c_void_p]; L.icet_stream.restype = C.c_void_p
    L.icet_device.argtypes = [C.c_void_p]; L.icet_device.restype = C.c_int
    for name in EXPORTED_SYMBOLS:
        getattr(L, name)
        if name not in _NON_STATUS:
            getattr(L, name).restype = C.c_int
    _lib = L
    return L


def _dev_scans(descs):
    """The icet_dev_scan array of (device_ptr, n, ld) triples (one entry even when there is none: ctypes has no empty array to pass)."""
    return (DevScan * max(len(descs), 1))(*[DevScan(int(p), int(n), int(ld)) for (p, n, ld) in descs])


def _vp(a):
    """An optional device pointer."""
    return C.c_void_p(a) if a else None


def _start_offsets(start_offsets, query):
    """The S x 6 float32 start offsets of a closure call (None: none), S as the query names it."""
    if start_offsets is None:
        return None
    off = np.ascontiguousarray(np.asarray(start_offsets, np.float32).reshape(-1, 6))
    if off.shape[0] != query.n_starts:
        raise IcetError(ICET_ERR_BAD_ARG, "start_offsets must hold n_starts rows of 6")
    return off


def _data(a):
    """The address of an optional host array."""
    return a.ctypes.data if a is not None else None


def _closure_dicts(recs, by_appearance, coarse):
    """One dict per closure record (CLOSURE_DTYPE): slot (None: no winner), reg, accepted, n_candidates, then stamp, d2, x0, X, pred_stds, cov, score, each None
    without a winner.  A query by appearance alone names its d2 ``distance`` and adds ``shift``; a coarse query adds ``coarse`` = dict(score, a, b, h) and,
    by appearance and only where there is a winner, ``distance`` and ``shift`` beside d2."""
    res = []
    for r in recs:
        win = r["slot"] >= 0
        d = dict(slot=int(r["slot"]) if win else None, reg=int(r["reg"]), accepted=bool(r["accepted"]), n_candidates=int(r["n_candidates"]))
        o = np.array(r["out"])
        v = {"stamp": int(r["stamp"]), "distance" if by_appearance and not coarse else "d2": float(r["d2"])}
        if by_appearance and not coarse:
            v["shift"] = int(r["reserved0"])
        v.update(x0=np.array(r["x0"]), X=o[:6].copy(), pred_stds=o[6:12].copy(), cov=o[12:48].reshape(6, 6).copy(),
                 score={n: r["score"][n].item() for n in ("chi2", "chi2_per_voxel", "voxels", "points_in", "points", "overlap")})
        if coarse:
            code = int(r["reserved1"][1])
            v["coarse"] = dict(score=int(r["reserved1"][0]), h=code & 255, a=((code >> 8) & 255) - 32, b=((code >> 16) & 255) - 32)
        d.update(v if win else dict.fromkeys(v))
        if coarse and by_appearance and win:
            d.update(distance=float(r["d2"]), shift=int(r["reserved0"]))
        res.append(d)
    return res


def _colmajor(scan):
    """N x 3 array-like -> float32 (3, N) C-contiguous buffer == column-major N x 3 (Eigen::MatrixXf::data())."""
    a = np.asarray(scan, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 3:
        raise IcetError(ICET_ERR_BAD_ARG, "scan must be N x 3")
    return np.ascontiguousarray(a.T)


def select_best(score, group, n_groups):
    """The rule of icet_select_best_device on the host (include/icet_hip.h): per group, among the registrations whose voxels reach
    max(1, ceil(0.5 x the group's largest)), the lowest chi2_per_voxel (NaN last), ties to the lowest index; -1 when none is eligible.
    ``score``: a dict of arrays or a SCORE_DTYPE array."""
    vox = np.asarray(score["voxels"]).astype(np.int64); cpv = np.asarray(score["chi2_per_voxel"], np.float32)
    group = np.asarray(group).reshape(-1)
    best = np.full(int(n_groups), -1, np.int32)
    for g in range(int(n_groups)):
        mem = np.nonzero(group == g)[0]
        if mem.size == 0:
            continue
        need = max(1, (int(vox[mem].max()) + 1) // 2)
        el = [r for r in mem if vox[r] >= need]
        if el:
            key = [(np.inf if np.isnan(cpv[r]) else float(cpv[r]), int(r)) for r in el]
            best[g] = min(key)[1]
    return best


class Context:
    """One device + stream + workspace (``icet_ctx``).  Not re-entrant; one per host thread."""

    def __init__(self, device=0, stream=None):
        L = load_library()
        h = C.c_void_p()
        st = L.icet_create(C.byref(h), int(device), C.c_void_p(stream) if stream else None)
        if st != ICET_OK:
            raise IcetError(st, "icet_create(device=%d)" % device)
        self._h = h
        self.device = device

    @classmethod
    def borrow(cls, handle, device=-1):
        """Wrap an icet_ctx* owned by someone else (e.g. icet_multi_context): never destroyed from here."""
        self = cls.__new__(cls)
        self._h = C.c_void_p(handle) if not isinstance(handle, C.c_void_p) else handle
        self.device = device
        self._borrowed = True
        return self

    def close(self):
        if getattr(self, "_borrowed", False):
            self._h = None
            return
        for ref in getattr(self, "_nodes", []):          # nodes borrow this context: they go first
            nd = ref()
            if nd is not None:
                nd.close()
        self._nodes = []
        if getattr(self, "_h", None):
            load_library().icet_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != ICET_OK:
            raise IcetError(st, load_library().icet_last_error(self._h).decode())

    def sync(self):
        self._check(load_library().icet_sync(self._h))

    def reserve(self, params, n_pairs, total_n1, total_n2):
        self._check(load_library().icet_reserve(self._h, C.byref(params), n_pairs, total_n1, total_n2))

    def debug_fetch(self, what, count):
        """Diagnostic: 'r' (float32, scan 1 in input order), 'bin' (uint16 per row: voxel id | literal-path flag << 14 | "r is exactly 0" << 15), 'src' (int32 scramble result), 'flags' (int32 per pair), 'lds_rank_ok' (count 1: the
        device passed the LDS-atomic order self-test of icet_create)."""
        code = {"r": 0, "bin": 1, "src": 3, "flags": 4, "rt2": 5, "lds_rank_ok": 6}[what]
        out = np.zeros(count, {0: np.float32, 1: np.uint16, 5: np.float32}.get(code, np.int32))
        self._check(load_library().icet_debug_fetch(self._h, code, out.ctypes.data, count))
        return out

    def keyframe_device(self, scan1_descs, params, d_rows_ptr=None):
        """Park the keyframe of the scans (device_ptr, n, ld) in this context (icet_keyframe_device[_n]: with d_rows_ptr -- a device int32
        array -- n is an upper bound and the actual row counts are read on the device)."""
        A = _dev_scans(scan1_descs)
        self._check(load_library().icet_keyframe_device_n(self._h, C.byref(params), len(scan1_descs), A, C.c_void_p(d_rows_ptr) if d_rows_ptr else None))

    def register_device(self, scan2_descs, params, d_out_ptr, d_x0_ptr=None, d_rows_ptr=None):
        """Gauss-Newton loop of the scans against the parked keyframe (icet_register_device[_n])."""
        B = _dev_scans(scan2_descs)
        self._check(load_library().icet_register_device_n(self._h, C.byref(params), len(scan2_descs), B, C.c_void_p(d_rows_ptr) if d_rows_ptr else None,
                                                          C.c_void_p(d_x0_ptr) if d_x0_ptr else None, C.c_void_p(d_out_ptr)))

    def register_indexed_device(self, kf_index, scan2_descs, params, d_out_ptr, d_x0_ptr=None):
        """Gauss-Newton loop of every scan 2 (device_ptr, n, ld) against the parked keyframe kf_index[r] (icet_register_indexed_device): repeats and
        any order allowed; d_out_ptr: device pointer to len(scan2_descs) x 48 floats.  The keyframe stays parked."""
        k = len(scan2_descs)
        idx = np.ascontiguousarray(np.asarray(kf_index, np.int32).reshape(-1))
        if idx.shape[0] != k:
            raise IcetError(ICET_ERR_BAD_ARG, "kf_index and scan2_descs differ in length")
        B = _dev_scans(scan2_descs)
        self._check(load_library().icet_register_indexed_device(self._h, C.byref(params), k, idx.ctypes.data, B,
                                                                C.c_void_p(d_x0_ptr) if d_x0_ptr else None, C.c_void_p(d_out_ptr)))

    def register_indexed_scored_device(self, kf_index, scan2_descs, params, d_out_ptr, d_score_ptr, d_x0_ptr=None):
        """register_indexed_device followed by the score at every final X (icet_register_indexed_scored_device): d_out carries the bits of the unscored
        call; d_score_ptr: device pointer to len(scan2_descs) icet_score records (32 bytes each, SCORE_DTYPE)."""
        k = len(scan2_descs)
        idx = np.ascontiguousarray(np.asarray(kf_index, np.int32).reshape(-1))
        if idx.shape[0] != k:
            raise IcetError(ICET_ERR_BAD_ARG, "kf_index and scan2_descs differ in length")
        B = _dev_scans(scan2_descs)
        self._check(load_library().icet_register_indexed_scored_device(self._h, C.byref(params), k, idx.ctypes.data, B,
                                                                       C.c_void_p(d_x0_ptr) if d_x0_ptr else None, C.c_void_p(d_out_ptr), C.c_void_p(d_score_ptr)))

    def score_indexed_device(self, kf_index, scan2_descs, params, d_X_ptr, d_score_ptr):
        """The score of scan 2 r at pose d_X[r] (device, len x 6 float32) against parked keyframe kf_index[r] (icet_score_indexed_device): no
        iteration; d_score_ptr: device pointer to len(scan2_descs) icet_score records."""
        k = len(scan2_descs)
        idx = np.ascontiguousarray(np.asarray(kf_index, np.int32).reshape(-1))
        if idx.shape[0] != k:
            raise IcetError(ICET_ERR_BAD_ARG, "kf_index and scan2_descs differ in length")
        B = _dev_scans(scan2_descs)
        self._check(load_library().icet_score_indexed_device(self._h, C.byref(params), k, idx.ctypes.data, B, C.c_void_p(d_X_ptr), C.c_void_p(d_score_ptr)))

    def select_best_device(self, group, n_groups, d_score_ptr, d_best_ptr, d_out_ptr=None, d_best_out_ptr=None):
        """The best registration of every group on the device (icet_select_best_device; the rule is in include/icet_hip.h): group[r] = the group of
        registration r (host, any order); d_best_ptr: device int32 x n_groups (-1: no eligible registration); d_best_out_ptr (optional): device
        n_groups x 48 floats, the winner's row of d_out_ptr."""
        g = np.ascontiguousarray(np.asarray(group, np.int32).reshape(-1))
        self._check(load_library().icet_select_best_device(self._h, g.shape[0], g.ctypes.data, int(n_groups), C.c_void_p(d_score_ptr),
                                                           C.c_void_p(d_out_ptr) if d_out_ptr else None, C.c_void_p(d_best_ptr),
                                                           C.c_void_p(d_best_out_ptr) if d_best_out_ptr else None))

    def set_option(self, name, value):
        """Launch-shape / diagnostic knob of this context (icet_set_option, include/icet_hip.h).  Launch-shape knobs leave the result
        bits alone; force_exact / guard_scale / lut_polar_quantile keep every decision but regroup float partial sums."""
        self._check(load_library().icet_set_option(self._h, name.encode(), float(value)))
        if name == "pg_solver":
            self._pg_solver = int(value)

    @contextlib.contextmanager
    def _pose_graph_solver(self, solver):
        """Option "pg_solver" for one call: ``solver`` None leaves the context's option alone; "cg", "direct", "auto" set it and put the old value back."""
        if solver is None:
            yield
            return
        if solver not in PG_SOLVERS:
            raise IcetError(ICET_ERR_BAD_ARG, 'solver must be None, "cg", "direct" or "auto"')
        old = getattr(self, "_pg_solver", PG_SOLVER_CG)
        self.set_option("pg_solver", PG_SOLVERS[solver])
        try:
            yield
        finally:
            self.set_option("pg_solver", old)

    def last_timing(self):
        t = np.zeros(4, np.float32)
        self._check(load_library().icet_last_timing(self._h, t.ctypes.data))
        return dict(keyframe_ms=float(t[0]), gn_loop_ms=float(t[1]), accumulate_ms=float(t[2]), accumulate_launches=int(t[3]))

    def last_timing_iters(self, cap=64):
        """Per-iteration HIP-event times (ms) of the point-pass launches of the last ICET_FLAG_TIMING call (icet_last_timing_iters)."""
        t = np.zeros(cap, np.float32); n = C.c_int32(0)
        self._check(load_library().icet_last_timing_iters(self._h, t.ctypes.data, cap, C.byref(n)))
        return t[:n.value].copy()

    def keep_stats(self, n_pairs):
        """The keep list of the point pass after the last throughput batch (icet_keep_stats): (n_pairs, 4) int32 = mode, groups kept, list passes, lists built."""
        out = np.zeros((n_pairs, 4), np.int32)
        self._check(load_library().icet_keep_stats(self._h, n_pairs, out.ctypes.data))
        return out

    def debug_pinv3(self, mats):
        """icet_debug_pinv3 (test hook): the 3 x 3 float COD pseudo-inverse of ICET_FLAG_REFERENCE_W on the device for n matrices (n, 3, 3) -> (n, 3, 3)."""
        A = np.ascontiguousarray(mats, np.float32).reshape(-1, 9)
        out = np.zeros_like(A)
        self._check(load_library().icet_debug_pinv3(self._h, A.ctypes.data, A.shape[0], out.ctypes.data))
        return out.reshape(-1, 3, 3)

    def debug_pinv3_double(self, packed):
        """icet_debug_pinv3_double (test hook): the 3 x 3 double pseudo-inverse of ICET_FLAG_DOUBLE_W on the device for n packed symmetric matrices
        (n, 6) = xx, xy, xz, yy, yz, zz -> (n, 6) in the same packing."""
        A = np.ascontiguousarray(packed, np.float32).reshape(-1, 6)
        out = np.zeros_like(A)
        self._check(load_library().icet_debug_pinv3_double(self._h, A.ctypes.data, A.shape[0], out.ctypes.data))
        return out

    def debug_point_sums(self, kf_index, scan2_descs, params, d_X_ptr, d_sums_ptr):
        """icet_debug_point_sums_device (test hook): the point pass of score_indexed_device at the poses d_X, then every voxel's raw accumulator record
        instead of the score.  d_sums_ptr: device pointer to len(scan2_descs) x V records of POINT_SUMS_DTYPE (80 bytes), indexed by voxel id."""
        k = len(scan2_descs)
        idx = np.ascontiguousarray(np.asarray(kf_index, np.int32).reshape(-1))
        if idx.shape[0] != k:
            raise IcetError(ICET_ERR_BAD_ARG, "kf_index and scan2_descs differ in length")
        B = _dev_scans(scan2_descs)
        self._check(load_library().icet_debug_point_sums_device(self._h, C.byref(params), k, idx.ctypes.data, B, C.c_void_p(d_X_ptr), C.c_void_p(d_sums_ptr)))

    def debug_gn_terms(self, kf_index, scan2_descs, params, d_X_ptr, d_sums_ptr, d_xf_ptr, d_htwh_ptr, d_htwdz_ptr, d_out_ptr):
        """icet_debug_gn_terms_device (test hook): debug_point_sums' point pass with the records left in place, then the production solve of iteration
        params.runlen - 1 on them.  Device pointers: d_sums (k x V records of POINT_SUMS_DTYPE), d_xf (k x 48 floats, the transform record), d_htwh (k x 36),
        d_htwdz (k x 6), d_out (k x 48: X | pred_stds | cov).  Returns after the stream has drained."""
        k = len(scan2_descs)
        idx = np.ascontiguousarray(np.asarray(kf_index, np.int32).reshape(-1))
        if idx.shape[0] != k:
            raise IcetError(ICET_ERR_BAD_ARG, "kf_index and scan2_descs differ in length")
        B = _dev_scans(scan2_descs)
        self._check(load_library().icet_debug_gn_terms_device(self._h, C.byref(params), k, idx.ctypes.data, B, C.c_void_p(d_X_ptr), C.c_void_p(d_sums_ptr),
                                                              C.c_void_p(d_xf_ptr), C.c_void_p(d_htwh_ptr), C.c_void_p(d_htwdz_ptr), C.c_void_p(d_out_ptr)))

    def debug_block_tridiag(self, diag, sub, rhs):
        """icet_debug_block_tridiag: x of the block-tridiagonal system (diag n x 6 x 6, sub n x 6 x 6 with sub[k] at (k, k - 1), rhs n x 6; doubles) through the
        device's block Cholesky factorisation and sweeps, and the status word (0: solved)."""
        D = np.ascontiguousarray(np.asarray(diag, np.float64).reshape(-1, 36)); n = D.shape[0]
        B = np.ascontiguousarray(np.asarray(sub, np.float64).reshape(n, 36)); r = np.ascontiguousarray(np.asarray(rhs, np.float64).reshape(n, 6))
        x = np.zeros((n, 6), np.float64); st = C.c_int32(-1)
        self._check(load_library().icet_debug_block_tridiag(self._h, n, D.ctypes.data, B.ctypes.data, r.ctypes.data, x.ctypes.data, C.byref(st)))
        return x, int(st.value)

    # ---- the pose graph: every call marshals its graph ONCE, through _pose_graph_host (host arrays) or _pose_graph_device (tensors) -----------------------------
    @staticmethod
    def _pose_graph_lists(n, closures, fixed, measurements=True):
        """ci, cj (int32), the closures' X and info (float32; None without ``measurements``: the caller has them as tensors) and fixed (uint8 or None)."""
        closures = list(closures)
        ci = np.ascontiguousarray([int(c[0]) for c in closures], np.int32); cj = np.ascontiguousarray([int(c[1]) for c in closures], np.int32)
        cX = cI = None
        if measurements:
            cX = np.ascontiguousarray([np.asarray(c[2], np.float32).reshape(6) for c in closures], np.float32).reshape(-1, 6)
            cI = np.ascontiguousarray([np.asarray(c[3], np.float32).reshape(36) for c in closures], np.float32).reshape(-1, 36)
        fx = None
        if fixed is not None:
            fx = np.ascontiguousarray(np.asarray(fixed).reshape(-1) != 0, np.uint8)
            if fx.shape[0] != n:
                raise IcetError(ICET_ERR_BAD_ARG, "fixed must hold one entry per pose")
        return ci, cj, cX, cI, fx

    def _pose_graph_args(self, n, poses, odo_X, odo_info, ci, cj, clo_X, clo_info, fx, ptr):
        """What a call site needs of a marshalled graph: ``n``, ``nc`` (the closure count) and ``args``, the eleven leading arguments of every
        icet_pose_graph_* entry, to splat.  ``keep`` holds the arrays behind those addresses: the caller keeps the object while the C call runs."""
        nc = ci.shape[0]
        return types.SimpleNamespace(n=n, nc=nc, keep=(poses, odo_X, odo_info, ci, cj, clo_X, clo_info, fx),
                                     args=(self._h, n, ptr(poses), ptr(odo_X), ptr(odo_info), nc, ci.ctypes.data, cj.ctypes.data, ptr(clo_X), ptr(clo_info), _data(fx)))

    def _pose_graph_host(self, poses, odo_X, odo_info, closures, fixed):
        """The graph of the five host-pointer calls (see _pose_graph_args): float32 rows, one of odo_X and odo_info per pose but the first."""
        P = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 16)); n = P.shape[0]
        oX = np.ascontiguousarray(np.asarray(odo_X, np.float32).reshape(-1, 6)); oI = np.ascontiguousarray(np.asarray(odo_info, np.float32).reshape(-1, 36))
        if n < 1 or oX.shape[0] != n - 1 or oI.shape[0] != n - 1:
            raise IcetError(ICET_ERR_BAD_ARG, "odo_X and odo_info must hold one row per pose but the first")
        return self._pose_graph_args(n, P, oX, oI, *self._pose_graph_lists(n, closures, fixed), lambda a: a.ctypes.data)

    def _pose_graph_device(self, poses, odo_X, odo_info, closures, fixed, clo_X, clo_info):
        """The graph of the two _device calls (see _pose_graph_args): contiguous float32 tensors on the device; the closures' X and info are uploaded from
        ``closures``, or are the tensors ``clo_X`` and ``clo_info``."""
        import torch
        for t in (poses, odo_X, odo_info):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise IcetError(ICET_ERR_BAD_ARG, "poses, odo_X and odo_info must be contiguous float32 tensors on the device")
        n = poses.numel() // 16
        if n < 1 or poses.numel() != n * 16 or odo_X.numel() != (n - 1) * 6 or odo_info.numel() != (n - 1) * 36:
            raise IcetError(ICET_ERR_BAD_ARG, "odo_X and odo_info must hold one row per pose but the first")
        ci, cj, cX, cI, fx = self._pose_graph_lists(n, closures, fixed, measurements=clo_X is None)
        if clo_X is None:
            clo_X = torch.from_numpy(cX).to(poses.device); clo_info = torch.from_numpy(cI).to(poses.device)
        else:
            for t in (clo_X, clo_info):
                if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                    raise IcetError(ICET_ERR_BAD_ARG, "clo_X and clo_info must be contiguous float32 tensors on the device")
            if clo_X.numel() != ci.shape[0] * 6 or clo_info.numel() != ci.shape[0] * 36:
                raise IcetError(ICET_ERR_BAD_ARG, "clo_X and clo_info must hold one row per closure")
        return self._pose_graph_args(n, poses, odo_X, odo_info, ci, cj, clo_X, clo_info, fx, lambda t: _vp(t.data_ptr()))

    @staticmethod
    def _pose_graph_result(res):
        return dict(chi2_initial=float(res.chi2_initial), chi2_final=float(res.chi2_final), status=int(res.status), gn_iterations=int(res.gn_iterations),
                    max_dx=float(res.max_dx), pcg_iterations=int(res.pcg_iterations), solver=int(res.solver))

    @staticmethod
    def _pose_graph_robust(robust, robust_scale=None, robust_odometry=False):
        """icet_pose_graph_robust of the three keyword arguments of the optimiser calls (``robust`` a name of PG_ROBUST_KINDS)."""
        if robust not in PG_ROBUST_KINDS:
            raise IcetError(ICET_ERR_BAD_ARG, 'robust must be None, "huber", "cauchy" or "geman_mcclure"')
        scale = PG_ROBUST_DEFAULT_SCALE if robust_scale is None else float(robust_scale)
        if not (scale > 0.0 and np.isfinite(scale)):
            raise IcetError(ICET_ERR_BAD_ARG, "robust_scale must be finite and positive")
        return PoseGraphRobust(PG_ROBUST_KINDS[robust], PG_ROBUST_ODOMETRY if robust_odometry else 0, scale)

    @classmethod
    def _pose_graph_robust_result(cls, res):
        return dict(cls._pose_graph_result(res.base), cost_initial=float(res.cost_initial), cost_final=float(res.cost_final), downweighted=int(res.downweighted))

    def optimize_pose_graph(self, poses, odo_X, odo_info, closures=(), fixed=None, gn_iters=10, dx_tol=1e-7, damping=0.0, max_pcg=0, pcg_tol=0.0, solver=None,
                            covariances=False, robust=None, robust_scale=None, robust_odometry=False):
        """icet_pose_graph_optimize: the poses (n x 4 x 4 float32) of a chain with odometry measurements ``odo_X`` ((n - 1) x 6) and information ``odo_info``
        ((n - 1) x 6 x 6) and the closure edges ``closures`` = (i, j, X, info) tuples as closure_edges returns them, optimised on the device.  Node 0 and the
        nodes with ``fixed[k] != 0`` stay.  Returns dict(poses n x 4 x 4 float32, poses64 n x 4 x 4, chi2_initial, chi2_final, status (POSE_GRAPH_*),
        gn_iterations, max_dx, edge_chi2 2 x E, pcg_iterations, solver).  A status of 2 or 3 is a result, not an error: the poses are then the inputs.
        ``solver``: None (the context's option "pg_solver"), "cg", "direct" or "auto" for this call; the result's ``solver`` is 1 when the direct solve ran --
        it ignores max_pcg and pcg_tol, and converges at the defaults where the closures' information is strong (closures from find_closures: use "auto").
        ``covariances``: True adds ``cov`` (n x 6 x 6) and ``cov_status``, pose_graph_marginals at the returned float32 poses.
        ``robust``: None, or "huber", "cauchy", "geman_mcclure": icet_pose_graph_optimize_robust, iteratively reweighted least squares with the threshold
        ``robust_scale`` in chi2 units (None: PG_ROBUST_DEFAULT_SCALE) on the closures, with ``robust_odometry`` on the odometry edges too.  The result then
        also has ``edge_weight`` (E: every edge's final weight), ``cost_initial``, ``cost_final`` (the robust objective; chi2_* stay the raw sums) and
        ``downweighted`` (the edges whose weight is below 0.5); its covariances are taken with the closures' information scaled by their weights
        (reweighted_closures; robust odometry weights are not applied there)."""
        closures = list(closures)
        g = self._pose_graph_host(poses, odo_X, odo_info, closures, fixed); n = g.n
        opt = PoseGraphOptions(int(gn_iters), int(max_pcg), float(dx_tol), float(damping), float(pcg_tol))
        out = np.zeros((n, 16), np.float32); p64 = np.zeros((n, 12), np.float64); chi = np.zeros((2, n - 1 + g.nc), np.float64)
        if robust is None:
            res = PoseGraphResult()
            with self._pose_graph_solver(solver):
                self._check(load_library().icet_pose_graph_optimize(*g.args, C.byref(opt), out.ctypes.data, p64.ctypes.data, chi.ctypes.data, C.byref(res)))
            r = self._pose_graph_result(res)
        else:
            rob = self._pose_graph_robust(robust, robust_scale, robust_odometry)
            wt = np.zeros(n - 1 + g.nc, np.float64); res = PoseGraphRobustResult()
            with self._pose_graph_solver(solver):
                self._check(load_library().icet_pose_graph_optimize_robust(*g.args, C.byref(opt), C.byref(rob), out.ctypes.data, p64.ctypes.data, chi.ctypes.data,
                                                                           wt.ctypes.data, C.byref(res)))
            r = dict(self._pose_graph_robust_result(res), edge_weight=wt)
        T64 = np.zeros((n, 4, 4)); T64[:, 3, 3] = 1.0; T64[:, :3, :3] = p64[:, :9].reshape(n, 3, 3); T64[:, :3, 3] = p64[:, 9:]
        r = dict(r, poses=out.reshape(n, 4, 4), poses64=T64, edge_chi2=chi)
        if covariances:
            if robust is not None:
                closures = reweighted_closures(closures, r["edge_weight"], n=n)
            mg = self.pose_graph_marginals(r["poses"], odo_X, odo_info, closures, fixed=fixed)
            r["cov"] = mg["cov"]; r["cov_status"] = mg["status"]
        return r

    def _pose_graph_marginals_result(self, res):
        return {k: int(getattr(res, k)) for k in ("status", "m", "factor_status", "wm_status", "ks_status")}

    def pose_graph_marginals(self, poses, odo_X, odo_info, closures=(), fixed=None):
        """icet_pose_graph_marginals: how well each pose of the graph is known.  The graph as optimize_pose_graph takes it, ``poses`` the poses to evaluate at
        (what the optimiser returned).  Returns dict(cov n x 6 x 6 float64, status, m, factor_status, wm_status, ks_status): block (k, k) of the inverse of the
        Gauss-Newton H at these poses, in the tangent of the right update T Exp(delta), delta = (translation in the node's own frame, rotation vector); a fixed
        node's block is zero.  pose_stds and position_cov_world read it.  A status of 2 (H is not positive definite) or 3 (not finite) is a result: every free
        node's block is then NaN.  More than 128 end nodes of closures off the band: IcetError(ICET_ERR_UNSUPPORTED)."""
        g = self._pose_graph_host(poses, odo_X, odo_info, closures, fixed)
        cov = np.zeros((g.n, 6, 6), np.float64); res = PoseGraphMarginalsResult()
        self._check(load_library().icet_pose_graph_marginals(*g.args, cov.ctypes.data, C.byref(res)))
        return dict(self._pose_graph_marginals_result(res), cov=cov)

    def pose_graph_marginals_device(self, poses, odo_X, odo_info, closures=(), fixed=None, clo_X=None, clo_info=None):
        """icet_pose_graph_marginals_device for torch tensors on this context's device, with the conventions of optimize_pose_graph_device.  Returns the dict of
        pose_graph_marginals with ``cov`` (n x 6 x 6 float64) as a tensor on the device.  The call returns when the result is known."""
        import torch
        g = self._pose_graph_device(poses, odo_X, odo_info, closures, fixed, clo_X, clo_info)
        cov = torch.zeros((g.n, 6, 6), dtype=torch.float64, device=poses.device); res = PoseGraphMarginalsResult()
        torch.cuda.current_stream(poses.device).synchronize()          # the context's stream is its own: the tensors must be complete
        self._check(load_library().icet_pose_graph_marginals_device(*g.args, _vp(cov.data_ptr()), C.byref(res)))
        return dict(self._pose_graph_marginals_result(res), cov=cov)

    @staticmethod
    def _pose_graph_targets(targets):
        t = np.ascontiguousarray(np.asarray(targets).reshape(-1), np.int32)
        if t.shape[0] < 1:
            raise IcetError(ICET_ERR_BAD_ARG, "targets must name at least one node")
        return t

    def pose_graph_covariance_columns(self, poses, odo_X, odo_info, closures=(), targets=(), fixed=None):
        """icet_pose_graph_covariance_columns: how well the poses are known relative to the ``targets`` (1 .. PG_MAX_TARGETS distinct nodes).  The graph as
        pose_graph_marginals takes it.  Returns dict(cols T x n x 6 x 6 float64, cov n x 6 x 6, status, m, factor_status, wm_status, ks_status): ``cols[t][k]`` is
        block (k, targets[t]) of the inverse of the Gauss-Newton H, rows node k's tangent and columns the target's; ``cov`` carries the bits of
        pose_graph_marginals, and so does ``cols[t][targets[t]]``.  A block that touches a fixed node is zero.  A status of 2 or 3 is a result: every block
        between two free nodes is then NaN.  relative_cov turns the blocks into the covariance of a function of two poses."""
        g = self._pose_graph_host(poses, odo_X, odo_info, closures, fixed)
        t = self._pose_graph_targets(targets)
        cols = np.zeros((t.shape[0], g.n, 6, 6), np.float64); cov = np.zeros((g.n, 6, 6), np.float64); res = PoseGraphMarginalsResult()
        self._check(load_library().icet_pose_graph_covariance_columns(*g.args, t.shape[0], t.ctypes.data, cols.ctypes.data, cov.ctypes.data, C.byref(res)))
        return dict(self._pose_graph_marginals_result(res), cols=cols, cov=cov)

    def pose_graph_covariance_columns_device(self, poses, odo_X, odo_info, closures=(), targets=(), fixed=None, clo_X=None, clo_info=None):
        """icet_pose_graph_covariance_columns_device for torch tensors on this context's device, with the conventions of pose_graph_marginals_device.  Returns
        the dict of pose_graph_covariance_columns with ``cols`` and ``cov`` as float64 tensors on the device.  The call returns when the result is known."""
        import torch
        g = self._pose_graph_device(poses, odo_X, odo_info, closures, fixed, clo_X, clo_info)
        t = self._pose_graph_targets(targets)
        cols = torch.zeros((t.shape[0], g.n, 6, 6), dtype=torch.float64, device=poses.device)
        cov = torch.zeros((g.n, 6, 6), dtype=torch.float64, device=poses.device); res = PoseGraphMarginalsResult()
        torch.cuda.current_stream(poses.device).synchronize()          # the context's stream is its own: the tensors must be complete
        self._check(load_library().icet_pose_graph_covariance_columns_device(*g.args, t.shape[0], t.ctypes.data, _vp(cols.data_ptr()), _vp(cov.data_ptr()), C.byref(res)))
        return dict(self._pose_graph_marginals_result(res), cols=cols, cov=cov)

    @staticmethod
    def _pose_graph_gate_result(res, threshold, d2, status):
        return dict(status=int(res.marg.status), m=int(res.marg.m), n_targets=int(res.n_targets), rejected=int(res.rejected), threshold=threshold,
                    accepted=(d2 < threshold) & (status == 0))

    def pose_graph_gate(self, poses, odo_X, odo_info, closures, candidates, fixed=None, threshold=None):
        """icet_pose_graph_gate: is each candidate closure plausible under what the graph knows?  The graph as pose_graph_marginals takes it; ``candidates`` is a
        list of (i, j, X, cov) -- keyframe node i seen from live node j with the measurement X and its 6 x 6 covariance, as closure_candidates returns them -- that
        are NOT edges of the graph yet (their noise would be counted twice).  Returns dict(d2 (the squared Mahalanobis distance of the residual under the
        covariance of the relative pose plus cov), res_cov n_cand x 6 x 6 (that covariance S), cand_status (0; 2: S is not positive definite; 3: not finite),
        accepted (d2 < threshold and cand_status 0), rejected, n_targets, threshold, status, m).  ``threshold``: None for PG_ROBUST_DEFAULT_SCALE, the 99 %
        quantile of chi2 with six degrees of freedom.  At most PG_GATE_MAX_CANDIDATES candidates with at most PG_MAX_TARGETS distinct live nodes per call."""
        candidates = list(candidates)
        g = self._pose_graph_host(poses, odo_X, odo_info, closures, fixed)
        gi, gj, cX, cC, _ = self._pose_graph_lists(g.n, candidates, None)
        nc = gi.shape[0]
        thr = PG_ROBUST_DEFAULT_SCALE if threshold is None else float(threshold)
        d2 = np.zeros(nc, np.float64); S = np.zeros((nc, 6, 6), np.float64); st = np.zeros(nc, np.int32); res = PoseGraphGateResult()
        self._check(load_library().icet_pose_graph_gate(*g.args, nc, gi.ctypes.data, gj.ctypes.data, cX.ctypes.data, cC.ctypes.data, thr, d2.ctypes.data, S.ctypes.data,
                                                        st.ctypes.data, C.byref(res)))
        thr = thr if thr > 0.0 else PG_ROBUST_DEFAULT_SCALE
        return dict(self._pose_graph_gate_result(res, thr, d2, st), d2=d2, res_cov=S, cand_status=st)

    def pose_graph_gate_device(self, poses, odo_X, odo_info, closures, gi, gj, cand_X, cand_cov, fixed=None, threshold=None, clo_X=None, clo_info=None):
        """icet_pose_graph_gate_device for torch tensors on this context's device, with the conventions of pose_graph_marginals_device: ``gi``, ``gj`` the
        candidates' nodes (host), ``cand_X`` (n_cand x 6) and ``cand_cov`` (n_cand x 6 x 6) contiguous float32 tensors on the device.  Returns the dict of
        pose_graph_gate with d2, res_cov, cand_status and accepted as tensors on the device.  The call returns when the result is known."""
        import torch
        g = self._pose_graph_device(poses, odo_X, odo_info, closures, fixed, clo_X, clo_info)
        gi = np.ascontiguousarray(np.asarray(gi).reshape(-1), np.int32); gj = np.ascontiguousarray(np.asarray(gj).reshape(-1), np.int32)
        nc = gi.shape[0]
        for t in (cand_X, cand_cov):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise IcetError(ICET_ERR_BAD_ARG, "cand_X and cand_cov must be contiguous float32 tensors on the device")
        if gj.shape[0] != nc or cand_X.numel() != nc * 6 or cand_cov.numel() != nc * 36:
            raise IcetError(ICET_ERR_BAD_ARG, "gi, gj, cand_X and cand_cov must hold one row per candidate")
        thr = PG_ROBUST_DEFAULT_SCALE if threshold is None else float(threshold)
        d2 = torch.zeros(nc, dtype=torch.float64, device=poses.device); S = torch.zeros((nc, 6, 6), dtype=torch.float64, device=poses.device)
        st = torch.zeros(nc, dtype=torch.int32, device=poses.device); res = PoseGraphGateResult()
        torch.cuda.current_stream(poses.device).synchronize()          # the context's stream is its own: the tensors must be complete
        self._check(load_library().icet_pose_graph_gate_device(*g.args, nc, gi.ctypes.data, gj.ctypes.data, _vp(cand_X.data_ptr()), _vp(cand_cov.data_ptr()), thr,
                                                               _vp(d2.data_ptr()), _vp(S.data_ptr()), _vp(st.data_ptr()), C.byref(res)))
        thr = thr if thr > 0.0 else PG_ROBUST_DEFAULT_SCALE
        return dict(self._pose_graph_gate_result(res, thr, d2, st), d2=d2, res_cov=S, cand_status=st)

    def debug_pose_graph_marginals(self, poses, odo_X, odo_info, closures=(), fixed=None):
        """icet_debug_pose_graph_marginals: pose_graph_marginals with its intermediate arrays.  Returns its dict with ends (m int32), D, B n x 6 x 6, A C x 6 x 6
        and band_cov n x 6 x 6 (the diagonal blocks of the band's inverse; NaN where the band did not factor)."""
        closures = list(closures)
        g = self._pose_graph_host(poses, odo_X, odo_info, closures, fixed); n, nc = g.n, g.nc
        m = len(pose_graph_ends(n, closures, fixed))
        arr = dict(D=np.full((n, 6, 6), np.nan), B=np.full((n, 6, 6), np.nan), A=np.full((nc, 6, 6), np.nan), band_cov=np.full((n, 6, 6), np.nan), cov=np.full((n, 6, 6), np.nan))
        ends = np.full(m, -1, np.int32)
        st = PoseGraphMarginalsDebug()
        for k in PoseGraphMarginalsDebug.ARRAYS:
            setattr(st, k, arr[k].ctypes.data)
        st.ends = ends.ctypes.data; st.ends_capacity = m
        self._check(load_library().icet_debug_pose_graph_marginals(*g.args, C.byref(st)))
        return dict(self._pose_graph_marginals_result(st.result), ends=ends, **arr)

    def debug_pose_graph_step(self, poses, odo_X, odo_info, closures=(), fixed=None, damping=0.0, max_pcg=0, pcg_tol=0.0, p=None):
        """icet_debug_pose_graph_step: the optimiser's first iteration on the device with its intermediate arrays, and q = H p for every vector of ``p``
        (K x n x 6 doubles).  Returns a dict of the arrays of icet_pose_graph_step (J E x 6 x 12, res E x 6, chi_start, chi_trial, D, B n x 6 x 6, A C x 6 x 6,
        g, x n x 6, Pt n x 12, q K x n x 6, cg_scalars band_solves x 2) and its scalars."""
        g = self._pose_graph_host(poses, odo_X, odo_info, closures, fixed); n, nc = g.n, g.nc; E = n - 1 + nc
        opt = PoseGraphOptions(1, int(max_pcg), 0.0, float(damping), float(pcg_tol))
        pv = np.zeros((0, n, 6)) if p is None else np.ascontiguousarray(np.asarray(p, np.float64).reshape(-1, n, 6))
        cap = int(max_pcg) if max_pcg > 0 else 12 * nc + 8
        arr = dict(J=np.zeros((E, 6, 12)), res=np.zeros((E, 6)), chi_start=np.zeros(E), chi_trial=np.zeros(E), D=np.zeros((n, 6, 6)), B=np.zeros((n, 6, 6)),
                   A=np.zeros((nc, 6, 6)), g=np.zeros((n, 6)), x=np.zeros((n, 6)), Pt=np.zeros((n, 12)), q=np.zeros(pv.shape), cg_scalars=np.full((cap, 2), np.nan))
        st = PoseGraphStep()
        for k in PoseGraphStep.ARRAYS:
            setattr(st, k, arr[k].ctypes.data)
        st.cg_capacity = cap
        self._check(load_library().icet_debug_pose_graph_step(*g.args, C.byref(opt), pv.shape[0], pv.ctypes.data, C.byref(st)))
        out = {k: int(getattr(st, k)) for k in ("factor_status", "cg_status", "band_solves", "cg_end", "cap", "c_offband", "trial")}
        out.update({k: float(getattr(st, k)) for k in ("chi2_start", "chi2_trial", "max_dx")})
        arr["cg_scalars"] = arr["cg_scalars"][:min(out["band_solves"], cap)]
        return dict(out, **arr)

    def debug_pose_graph_direct(self, poses, odo_X, odo_info, closures=(), fixed=None, damping=0.0, p=None):
        """icet_debug_pose_graph_direct: the optimiser's first iteration with the DIRECT solve on the device, its intermediate arrays copied out, and q = H p
        for every vector of ``p``.  Returns a dict: ends (m int32), D, B n x 6 x 6, A C x 6 x 6, g, x0, x n x 6, Z 6n x q, Wm, L, Ks, Lk q x q (q = 6 m), Pt
        n x 12, chi_trial, q K x n x 6, and the scalars of icet_pose_graph_direct_step."""
        closures = list(closures)
        g = self._pose_graph_host(poses, odo_X, odo_info, closures, fixed); n, nc = g.n, g.nc; E = n - 1 + nc
        opt = PoseGraphOptions(1, 0, 0.0, float(damping), 0.0)
        m = len(pose_graph_ends(n, closures, fixed)); q = 6 * m
        pv = np.zeros((0, n, 6)) if p is None else np.ascontiguousarray(np.asarray(p, np.float64).reshape(-1, n, 6))
        nan = lambda *shape: np.full(shape, np.nan)      # noqa: E731
        arr = dict(D=nan(n, 6, 6), B=nan(n, 6, 6), A=nan(nc, 6, 6), g=nan(n, 6), Z=nan(6 * n, q), Wm=nan(q, q), L=nan(q, q), Ks=nan(q, q), Lk=nan(q, q), x0=nan(n, 6),
                   x=nan(n, 6), Pt=nan(n, 12), chi_trial=nan(E), q=np.zeros(pv.shape))
        ends = np.full(m, -1, np.int32)
        st = PoseGraphDirectStep()
        for k in PoseGraphDirectStep.ARRAYS:
            setattr(st, k, arr[k].ctypes.data)
        st.ends = ends.ctypes.data; st.ends_capacity = m
        self._check(load_library().icet_debug_pose_graph_direct(*g.args, C.byref(opt), pv.shape[0], pv.ctypes.data, C.byref(st)))
        out = {k: int(getattr(st, k)) for k in ("m", "factor_status", "wm_status", "ks_status", "band_solves", "trial")}
        out.update({k: float(getattr(st, k)) for k in ("chi2_start", "chi2_trial", "max_dx")})
        return dict(out, ends=ends, **arr)

    def optimize_pose_graph_device(self, poses, odo_X, odo_info, closures=(), fixed=None, gn_iters=10, dx_tol=1e-7, damping=0.0, max_pcg=0, pcg_tol=0.0,
                                   clo_X=None, clo_info=None, solver=None, robust=None, robust_scale=None, robust_odometry=False):
        """icet_pose_graph_optimize_device for torch tensors on this context's device: ``poses`` n x 4 x 4, ``odo_X`` (n - 1) x 6, ``odo_info`` (n - 1) x 6 x 6,
        float32 and contiguous.  ``closures`` as in optimize_pose_graph (their X and info are uploaded), or (i, j) pairs with ``clo_X`` C x 6 and ``clo_info``
        C x 6 x 6 as float32 tensors.  Returns the dict of optimize_pose_graph with poses (float32), poses64 (n x 12 float64: R row-major, then t) and edge_chi2
        (2 x E float64) as tensors on the device.  ``solver`` as in optimize_pose_graph.  The call returns when the result is known.
        ``robust``, ``robust_scale``, ``robust_odometry`` as in optimize_pose_graph: icet_pose_graph_optimize_robust_device; ``edge_weight`` (E float64) is then
        a tensor on the device."""
        import torch
        g = self._pose_graph_device(poses, odo_X, odo_info, closures, fixed, clo_X, clo_info); n = g.n
        opt = PoseGraphOptions(int(gn_iters), int(max_pcg), float(dx_tol), float(damping), float(pcg_tol))
        out = torch.zeros((n, 4, 4), dtype=torch.float32, device=poses.device); p64 = torch.zeros((n, 12), dtype=torch.float64, device=poses.device)
        chi = torch.zeros((2, n - 1 + g.nc), dtype=torch.float64, device=poses.device)
        rob = None if robust is None else self._pose_graph_robust(robust, robust_scale, robust_odometry)
        wt = None if robust is None else torch.zeros(n - 1 + g.nc, dtype=torch.float64, device=poses.device)
        torch.cuda.current_stream(poses.device).synchronize()          # the context's stream is its own: the tensors must be complete
        outs = (_vp(out.data_ptr()), _vp(p64.data_ptr()), _vp(chi.data_ptr()))
        with self._pose_graph_solver(solver):
            if robust is None:
                res = PoseGraphResult()
                self._check(load_library().icet_pose_graph_optimize_device(*g.args, C.byref(opt), *outs, C.byref(res)))
                r = self._pose_graph_result(res)
            else:
                res = PoseGraphRobustResult()
                self._check(load_library().icet_pose_graph_optimize_robust_device(*g.args, C.byref(opt), C.byref(rob), *outs, _vp(wt.data_ptr()), C.byref(res)))
                r = dict(self._pose_graph_robust_result(res), edge_weight=wt)
        return dict(r, poses=out, poses64=p64, edge_chi2=chi)

    def debug_fix(self, values):
        """icet_debug_fix (test hook): n floats through the point pass's float -> 2^36 fixed-point conversions -> (n, 3) uint64 = to_fix_biased (defined for
        |v| < 2^15), to_fix_wide_biased, to_fix."""
        v = np.ascontiguousarray(values, np.float32).reshape(-1)
        out = np.zeros((v.shape[0], 3), np.uint64)
        self._check(load_library().icet_debug_fix(self._h, v.ctypes.data, v.shape[0], out.ctypes.data))
        return out

    def debug_spherical(self, xyz, num_bins_theta=75, num_bins_phi=24):
        """icet_debug_spherical (test hook): N x 3 rows through the device functions of the shared arithmetic rule.  Returns dict of float32 (N, k) arrays (voxel: int32
        (N,)): sph = r | theta | phi of c2s_cr, voxel = voxel_of(theta, phi), rt_any = x | y | z of roundtrip_any, cr_ang = theta | phi and cr = x | y | z of
        roundtrip_cr called directly (NaN for rows whose r is 0 or not finite)."""
        s = _colmajor(xyz); n = s.shape[1]
        out = np.zeros((12, n), np.float32)
        self._check(load_library().icet_debug_spherical(self._h, s.ctypes.data, n, n, int(num_bins_theta), int(num_bins_phi), out.ctypes.data))
        return dict(sph=out[0:3].T.copy(), voxel=out[3].view(np.int32).copy(), rt_any=out[4:7].T.copy(), cr_ang=out[7:9].T.copy(), cr=out[9:12].T.copy())

    def debug_gn_tail(self, htwh, htwdz):
        """icet_debug_gn_tail (test hook): the 6x6 tail of an iteration on the device for n (HTWH, HTWdz).  Returns dict of arrays with leading dimension n:
        cov (6, 6), pred_stds, dx, eigvals (NaN on the Cholesky route), pruned, route."""
        H = np.ascontiguousarray(htwh, np.float32).reshape(-1, 36); g = np.ascontiguousarray(htwdz, np.float32).reshape(-1, 6)
        n = H.shape[0]
        out = np.zeros((n, 56), np.float32)
        self._check(load_library().icet_debug_gn_tail(self._h, H.ctypes.data, g.ctypes.data, n, out.ctypes.data))
        return dict(cov=out[:, :36].reshape(n, 6, 6), pred_stds=out[:, 36:42], dx=out[:, 42:48], eigvals=out[:, 48:54], pruned=out[:, 54].astype(np.int32), route=out[:, 55].astype(np.int32))


    # -- single pair, host arrays ---------------------------------------------------------------
    def solve(self, scan1, scan2, runlen, X0, num_bins_phi, num_bins_theta, n=25, thresh=0.1, buff=0.1, aux=False, flags=0):
        """icet_solve.  scan1 / scan2: N x 3 (any layout numpy can view; an N x 3 array in Fortran order -- an Eigen::MatrixXf -- is
        passed without a copy).  aux=True also returns the side tables (icet_aux), among them ``points2`` (N2 x 3); aux="full" adds the
        per-point members of the reference object (points1_spherical, point_index1 / bin_start1, points2_spherical, voxel2)."""
        s1, s2 = _colmajor(scan1), _colmajor(scan2)
        p = Params(int(runlen), int(num_bins_phi), int(num_bins_theta), int(n), float(thresh), float(buff), int(flags))
        x0 = np.asarray(X0, np.float32).reshape(6).copy()
        X = np.zeros(6, np.float32); ps = np.zeros(6, np.float32); cov = np.zeros(36, np.float32)
        out = {}
        auxs = None
        if aux:
            V = int(num_bins_phi) * int(num_bins_theta); rl = max(int(runlen), 1)
            arr = dict(cluster_bounds=np.zeros((V, 6), np.float32), n1_raw=np.zeros(V, np.int32), has_fit=np.zeros(V, np.int32),
                       mu1=np.zeros((V, 3), np.float32), sigma1=np.zeros((V, 3, 3), np.float32), evecs1=np.zeros((V, 3, 3), np.float32),
                       l_diag=np.zeros((V, 3), np.float32), x_hist=np.zeros((rl, 6), np.float32), htwh=np.zeros((rl, 6, 6), np.float32),
                       htwdz=np.zeros((rl, 6), np.float32), n2_raw=np.zeros((rl, V), np.int32), n2_in=np.zeros((rl, V), np.int32),
                       test_points=np.zeros((V, 6, 3), np.float32), points2=np.zeros((3, s2.shape[1]), np.float32),
                       cond_info=np.zeros((rl, 8), np.float32))
            if aux == "full":
                arr.update(points1_spherical=np.zeros((3, s1.shape[1]), np.float32), point_index1=np.zeros(s1.shape[1], np.int32), bin_start1=np.zeros(V + 1, np.int32),
                           points2_spherical=np.zeros((3, s2.shape[1]), np.float32), voxel2=np.zeros(s2.shape[1], np.int32))
            auxs = Aux()
            for k, v in arr.items():
                setattr(auxs, k, v.ctypes.data_as(_I if v.dtype == np.int32 else _F))
            for k in ("points2", "points1_spherical", "points2_spherical"):
                if k in arr:
                    arr[k] = arr[k].T                         # (N, 3) views of the column-major buffers
            out["aux"] = arr
        st = load_library().icet_solve(self._h, C.byref(p), s1.ctypes.data, s1.shape[1], s1.shape[1], s2.ctypes.data, s2.shape[1], s2.shape[1],
                                       x0.ctypes.data, X.ctypes.data, ps.ctypes.data, cov.ctypes.data, C.byref(auxs) if auxs is not None else None)
        self._check(st)
        out.update(X=X, pred_stds=ps, cov=cov.reshape(6, 6))
        return out

    # -- batch, host arrays ------------------------------------------------------------------------
    def solve_batch(self, scans1, scans2, runlen, X0=None, num_bins_phi=24, num_bins_theta=75, n=25, thresh=0.1, buff=0.1):
        k = len(scans1)
        if len(scans2) != k:
            raise IcetError(ICET_ERR_BAD_ARG, "scans1 and scans2 differ in length")
        p = Params(int(runlen), int(num_bins_phi), int(num_bins_theta), int(n), float(thresh), float(buff), 0)
        s1 = [_colmajor(s) for s in scans1]; s2 = [_colmajor(s) for s in scans2]
        a1 = (C.c_void_p * max(k, 1))(*[s.ctypes.data for s in s1]); a2 = (C.c_void_p * max(k, 1))(*[s.ctypes.data for s in s2])
        n1 = np.array([s.shape[1] for s in s1], np.int64); n2 = np.array([s.shape[1] for s in s2], np.int64)
        x0 = None if X0 is None else np.ascontiguousarray(np.asarray(X0, np.float32).reshape(k, 6))
        X = np.zeros((k, 6), np.float32); ps = np.zeros((k, 6), np.float32); cov = np.zeros((k, 36), np.float32)
        st = load_library().icet_solve_batch(self._h, C.byref(p), k, a1, n1.ctypes.data, a2, n2.ctypes.data,
                                             x0.ctypes.data if x0 is not None else None, X.ctypes.data, ps.ctypes.data, cov.ctypes.data)
        self._check(st)
        return dict(X=X, pred_stds=ps, cov=cov.reshape(k, 6, 6))

    # -- many scans against shared keyframes, host arrays ------------------------------------------------
    def solve_indexed(self, scans1, scans2, kf_index, runlen, X0=None, num_bins_phi=24, num_bins_theta=75, n=25, thresh=0.1, buff=0.1, flags=0):
        """icet_solve_indexed: registration r solves (scans1[kf_index[r]], scans2[r]) from X0[r], each keyframe built once.  The keyframes stay
        parked in this context.  Returns X, pred_stds and cov per registration, like solve_batch."""
        k = len(scans2)
        idx = np.ascontiguousarray(np.asarray(kf_index, np.int32).reshape(-1))
        if idx.shape[0] != k:
            raise IcetError(ICET_ERR_BAD_ARG, "kf_index and scans2 differ in length")
        p = Params(int(runlen), int(num_bins_phi), int(num_bins_theta), int(n), float(thresh), float(buff), int(flags))
        s1 = [_colmajor(s) for s in scans1]; s2 = [_colmajor(s) for s in scans2]
        a1 = (C.c_void_p * max(len(s1), 1))(*[s.ctypes.data for s in s1]); a2 = (C.c_void_p * max(k, 1))(*[s.ctypes.data for s in s2])
        n1 = np.array([s.shape[1] for s in s1], np.int64); n2 = np.array([s.shape[1] for s in s2], np.int64)
        x0 = None if X0 is None else np.ascontiguousarray(np.asarray(X0, np.float32).reshape(k, 6))
        X = np.zeros((k, 6), np.float32); ps = np.zeros((k, 6), np.float32); cov = np.zeros((k, 36), np.float32)
        st = load_library().icet_solve_indexed(self._h, C.byref(p), len(s1), a1, n1.ctypes.data, k, idx.ctypes.data, a2, n2.ctypes.data,
                                               x0.ctypes.data if x0 is not None else None, X.ctypes.data, ps.ctypes.data, cov.ctypes.data)
        self._check(st)
        return dict(X=X, pred_stds=ps, cov=cov.reshape(k, 6, 6))

    def solve_indexed_scored(self, scans1, scans2, kf_index, runlen, X0=None, num_bins_phi=24, num_bins_theta=75, n=25, thresh=0.1, buff=0.1, flags=0):
        """icet_solve_indexed_scored: what solve_indexed returns plus ``score``, a dict of arrays (chi2, chi2_per_voxel, voxels, points_in, points,
        overlap) with the score of every registration at its final X."""
        k = len(scans2)
        idx = np.ascontiguousarray(np.asarray(kf_index, np.int32).reshape(-1))
        if idx.shape[0] != k:
            raise IcetError(ICET_ERR_BAD_ARG, "kf_index and scans2 differ in length")
        p = Params(int(runlen), int(num_bins_phi), int(num_bins_theta), int(n), float(thresh), float(buff), int(flags))
        s1 = [_colmajor(s) for s in scans1]; s2 = [_colmajor(s) for s in scans2]
        a1 = (C.c_void_p * max(len(s1), 1))(*[s.ctypes.data for s in s1]); a2 = (C.c_void_p * max(k, 1))(*[s.ctypes.data for s in s2])
        n1 = np.array([s.shape[1] for s in s1], np.int64); n2 = np.array([s.shape[1] for s in s2], np.int64)
        x0 = None if X0 is None else np.ascontiguousarray(np.asarray(X0, np.float32).reshape(k, 6))
        X = np.zeros((k, 6), np.float32); ps = np.zeros((k, 6), np.float32); cov = np.zeros((k, 36), np.float32)
        sc = np.zeros(k, SCORE_DTYPE)
        st = load_library().icet_solve_indexed_scored(self._h, C.byref(p), len(s1), a1, n1.ctypes.data, k, idx.ctypes.data, a2, n2.ctypes.data,
                                                      x0.ctypes.data if x0 is not None else None, X.ctypes.data, ps.ctypes.data, cov.ctypes.data, sc.ctypes.data)
        self._check(st)
        return dict(X=X, pred_stds=ps, cov=cov.reshape(k, 6, 6), score=scores_as_dict(sc))

    def score_indexed(self, scans1, scans2, kf_index, X, num_bins_phi=24, num_bins_theta=75, n=25, thresh=0.1, buff=0.1, flags=0, runlen=0):
        """icet_score_indexed: the score of scans2[r] at pose X[r] against scans1[kf_index[r]] (no iteration; ``runlen`` only places the moving-voxel
        gate of FLAG_REJECT_MOVING).  The keyframes stay parked.  Returns a dict of arrays like solve_indexed_scored's ``score``."""
        k = len(scans2)
        idx = np.ascontiguousarray(np.asarray(kf_index, np.int32).reshape(-1))
        if idx.shape[0] != k:
            raise IcetError(ICET_ERR_BAD_ARG, "kf_index and scans2 differ in length")
        x = np.ascontiguousarray(np.asarray(X, np.float32))
        if x.size != 6 * k:
            raise IcetError(ICET_ERR_BAD_ARG, "X must hold 6 floats per registration")
        p = Params(int(runlen), int(num_bins_phi), int(num_bins_theta), int(n), float(thresh), float(buff), int(flags))
        s1 = [_colmajor(s) for s in scans1]; s2 = [_colmajor(s) for s in scans2]
        a1 = (C.c_void_p * max(len(s1), 1))(*[s.ctypes.data for s in s1]); a2 = (C.c_void_p * max(k, 1))(*[s.ctypes.data for s in s2])
        n1 = np.array([s.shape[1] for s in s1], np.int64); n2 = np.array([s.shape[1] for s in s2], np.int64)
        sc = np.zeros(k, SCORE_DTYPE)
        st = load_library().icet_score_indexed(self._h, C.byref(p), len(s1), a1, n1.ctypes.data, k, idx.ctypes.data, a2, n2.ctypes.data,
                                               x.ctypes.data, sc.ctypes.data)
        self._check(st)
        return scores_as_dict(sc)

    def solve_multistart(self, scan1, scan2, starts, runlen, num_bins_phi=24, num_bins_theta=75, n=25, thresh=0.1, buff=0.1, flags=0):
        """One pair from several starts (``starts``: k x 6 X0), each solved and scored against the one keyframe of scan1; the start chosen by the rule of
        icet_select_best_device (include/icet_hip.h).  Returns dict(best, X, pred_stds, cov, score, X_all): ``best`` is the chosen start's index
        (-1 when no start has a contributing voxel: X, pred_stds and cov are then None), ``score`` every start's score (named arrays), X_all every final X."""
        x0 = np.ascontiguousarray(np.asarray(starts, np.float32).reshape(-1, 6))
        k = x0.shape[0]
        res = self.solve_indexed_scored([scan1], [scan2] * k, [0] * k, runlen, X0=x0, num_bins_phi=num_bins_phi, num_bins_theta=num_bins_theta,
                                        n=n, thresh=thresh, buff=buff, flags=flags)
        best = select_best(res["score"], np.zeros(k, np.int32), 1)[0]
        out = dict(best=int(best), score=res["score"], X_all=res["X"])
        if best < 0:
            out.update(X=None, pred_stds=None, cov=None)
        else:
            out.update(X=res["X"][best].copy(), pred_stds=res["pred_stds"][best].copy(), cov=res["cov"][best].copy())
        return out

    # -- batch, device-resident (raw device pointers; torch is only the allocator in callers) ---------
    def solve_batch_device(self, scan1_descs, scan2_descs, params, d_out_ptr, d_x0_ptr=None):
        """scan*_descs: sequences of (device_ptr, n, ld).  d_out_ptr: device pointer to n_pairs x 48 floats."""
        k = len(scan1_descs)
        A = _dev_scans(scan1_descs)
        B = _dev_scans(scan2_descs)
        st = load_library().icet_solve_batch_device(self._h, C.byref(params), k, A, B,
                                                    C.c_void_p(d_x0_ptr) if d_x0_ptr else None, C.c_void_p(d_out_ptr))
        self._check(st)


class KeyframeStore:
    """``icet_keyframe_store`` (include/icet_hip.h): slots of keyframes built once and kept on ``ctx``'s device, whatever else runs on the context;
    scans register and are scored against any set of slots.  The store borrows ``ctx`` (closed before it)."""

    def __init__(self, ctx, capacity, num_bins_phi=24, num_bins_theta=75, n=25, thresh=0.1, buff=0.1, flags=0):
        self._ctx = ctx
        self.params = Params(0, int(num_bins_phi), int(num_bins_theta), int(n), float(thresh), float(buff), int(flags))
        h = C.c_void_p()
        st = load_library().icet_keyframe_store_create(ctx._h, C.byref(self.params), int(capacity), C.byref(h))
        if st != ICET_OK:
            raise IcetError(st, "icet_keyframe_store_create: " + load_library().icet_last_error(ctx._h).decode())
        self._h = h
        self.V = int(num_bins_phi) * int(num_bins_theta)
        self.appearance = None                                        # AppearanceParams once enable_appearance has run
        self.coarse = None                                            # CoarseParams once enable_coarse has run
        import weakref
        if not hasattr(ctx, "_nodes"):
            ctx._nodes = []
        ctx._nodes.append(weakref.ref(self))

    def close(self):
        if getattr(self, "_h", None):
            # (a context finalised first -- both in one garbage cycle, whose weak references are cleared before any finaliser runs -- took the
            # device with it: the store's memory goes with the process then; destroying it would touch the freed context)
            if getattr(self._ctx, "_h", None):
                load_library().icet_keyframe_store_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != ICET_OK:
            raise IcetError(st, load_library().icet_keyframe_store_last_error(self._h).decode())

    def _params(self, runlen, flags):
        q = self.params
        return Params(int(runlen), q.bins_phi, q.bins_theta, q.n, q.thresh, q.buff, (q.flags & (FLAG_TRUE_SORT | FLAG_HALF_GAP_BOUNDS)) | int(flags))

    @staticmethod
    def _index(slot_index, k):
        idx = np.ascontiguousarray(np.asarray(slot_index, np.int32).reshape(-1))
        if idx.shape[0] != k:
            raise IcetError(ICET_ERR_BAD_ARG, "slot_index and scan2_descs differ in length")
        return idx

    def reserve(self, capacity):
        self._check(load_library().icet_keyframe_store_reserve(self._h, int(capacity)))

    def put_device(self, slots, scan1_descs, d_rows_ptr=None):
        """Build the keyframes of the scans (device_ptr, n, ld) and park keyframe k in slot slots[k] (icet_keyframe_store_put_device; with d_rows_ptr
        -- a device int32 array -- n is an upper bound and the actual row counts are read on the device).  Asynchronous on the context's stream."""
        k = len(scan1_descs)
        sl = self._index(slots, k)
        A = _dev_scans(scan1_descs)
        self._check(load_library().icet_keyframe_store_put_device(self._h, k, sl.ctypes.data, A, C.c_void_p(d_rows_ptr) if d_rows_ptr else None))

    def put(self, slots, scans):
        """put_device for host N x 3 arrays: staged on the device; returns once the put has run."""
        import torch
        dev = torch.device("cuda", self._ctx.device)
        bufs = [torch.from_numpy(_colmajor(s)).to(dev) for s in scans]
        torch.cuda.synchronize(dev)
        self.put_device(slots, [(b.data_ptr(), b.shape[1], b.shape[1]) for b in bufs])
        self._ctx.sync()

    def put_from_map(self, slots, vmap, poses, max_range, min_range=0.0, min_points=1, cap_rows=None, stamps=None, static=False):
        """Fill slots[k] with the sub-map of ``vmap`` (a VoxelMap on the same context) around poses[k], in that pose's frame: VoxelMap.query_device into buffers
        the store object keeps alive, then put_device with the query's d_rows -- the row counts never visit the host, and nothing synchronises between the two.
        cap_rows: the rows reserved per sub-map (None: the cells the map's index holds, which no sub-map exceeds; a smaller value truncates to the lowest
        keys).  With ``stamps`` the slots also get ``poses`` and the stamps (set_pose).  ``static``: without the cells the map's current evidence calls transient
        (VoxelMap.evidence).  Returns the device int32 tensors (rows, total, status)."""
        import torch
        dev = torch.device("cuda", self._ctx.device)
        T = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 16))
        k = T.shape[0]
        sl = self._index(slots, k)
        cap = max(int(vmap.index()["cells_out"]) if cap_rows is None else int(cap_rows), 1)
        xyz = torch.zeros((k, 3, cap), dtype=torch.float32, device=dev)
        words = torch.zeros((3, k), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)                                   # (the buffers are complete before the context's stream writes them)
        self._map_bufs = (xyz, words)                                 # alive until the next call: the put reads them in stream order
        vmap.query_device(T, [(xyz[j].data_ptr(), cap, cap) for j in range(k)], words[0].data_ptr(), min_range=min_range, max_range=max_range,
                          min_points=min_points, d_total_ptr=words[1].data_ptr(), d_status_ptr=words[2].data_ptr(), static=static)
        self.put_device(sl, [(xyz[j].data_ptr(), cap, cap) for j in range(k)], words[0].data_ptr())
        if stamps is not None:
            self.set_pose(sl, T, stamps)
        return words[0], words[1], words[2]

    def register_device(self, slot_index, scan2_descs, params, d_out_ptr, d_x0_ptr=None):
        """Context.register_indexed_device against the store's slots (icet_keyframe_store_register_device)."""
        k = len(scan2_descs)
        idx = self._index(slot_index, k)
        B = _dev_scans(scan2_descs)
        self._check(load_library().icet_keyframe_store_register_device(self._h, C.byref(params), k, idx.ctypes.data, B,
                                                                       C.c_void_p(d_x0_ptr) if d_x0_ptr else None, C.c_void_p(d_out_ptr)))

    def register_scored_device(self, slot_index, scan2_descs, params, d_out_ptr, d_score_ptr, d_x0_ptr=None):
        """Context.register_indexed_scored_device against the store's slots (icet_keyframe_store_register_scored_device)."""
        k = len(scan2_descs)
        idx = self._index(slot_index, k)
        B = _dev_scans(scan2_descs)
        self._check(load_library().icet_keyframe_store_register_scored_device(self._h, C.byref(params), k, idx.ctypes.data, B,
                                                                              C.c_void_p(d_x0_ptr) if d_x0_ptr else None, C.c_void_p(d_out_ptr), C.c_void_p(d_score_ptr)))

    def score_device(self, slot_index, scan2_descs, params, d_X_ptr, d_score_ptr):
        """Context.score_indexed_device against the store's slots (icet_keyframe_store_score_device)."""
        k = len(scan2_descs)
        idx = self._index(slot_index, k)
        B = _dev_scans(scan2_descs)
        self._check(load_library().icet_keyframe_store_score_device(self._h, C.byref(params), k, idx.ctypes.data, B, C.c_void_p(d_X_ptr), C.c_void_p(d_score_ptr)))

    def debug_fetch(self, slot, what, count=None):
        """Diagnostic: one occupied slot's tables -- 'n_slots' (int), 'hot' ((n_slots, 12) words of SlotHot), 'fit' ((n_slots, 20) words of SlotFit),
        'slot_of_voxel' (int16, V), 'pose' (4 x 4 float32, NaN entries without a pose), 'stamp' (int; -1 without a pose), 'descriptor' ((rings, sectors)
        uint8) and 'weights' ((sectors) float32) of a store with appearance enabled, 'grid' ((cells, cells / 32) uint32) of a store with coarse alignment
        enabled.  Words are returned as uint32 (view them as float32 / int32)."""
        L = load_library()
        if what == "grid":
            if self.coarse is None:
                raise IcetError(ICET_ERR_BAD_ARG, "coarse alignment is not enabled on this store")
            out = np.zeros((self.coarse.cells, self.coarse.cells // 32), np.uint32)
            self._check(L.icet_keyframe_store_debug_fetch(self._h, int(slot), 8, out.ctypes.data, out.size))
            return out
        if what in ("descriptor", "weights"):
            if self.appearance is None:
                raise IcetError(ICET_ERR_BAD_ARG, "appearance is not enabled on this store")
            a = self.appearance
            out = np.zeros((a.rings, a.sectors), np.uint8) if what == "descriptor" else np.zeros(a.sectors, np.float32)
            self._check(L.icet_keyframe_store_debug_fetch(self._h, int(slot), 6 if what == "descriptor" else 7, out.ctypes.data, out.size))
            return out
        if what == "pose":
            out = np.zeros(16, np.float32)
            self._check(L.icet_keyframe_store_debug_fetch(self._h, int(slot), 4, out.ctypes.data, 16))
            return out.reshape(4, 4)
        if what == "stamp":
            out = np.zeros(1, np.int64)
            self._check(L.icet_keyframe_store_debug_fetch(self._h, int(slot), 5, out.ctypes.data, 1))
            return int(out[0])
        ns = np.zeros(1, np.int32)
        self._check(L.icet_keyframe_store_debug_fetch(self._h, int(slot), 0, ns.ctypes.data, 1))
        ns = int(ns[0])
        if what == "n_slots":
            return ns
        if what == "slot_of_voxel":
            out = np.zeros(self.V if count is None else int(count), np.int16)
            self._check(L.icet_keyframe_store_debug_fetch(self._h, int(slot), 3, out.ctypes.data, out.size))
            return out
        code, words = {"hot": (1, 12), "fit": (2, 20)}[what]
        out = np.zeros(ns * words if count is None else int(count), np.uint32)
        self._check(L.icet_keyframe_store_debug_fetch(self._h, int(slot), code, out.ctypes.data, out.size))
        return out.reshape(-1, words) if count is None else out

    @staticmethod
    def _poses(poses, stamps):
        T = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 16))
        st = np.ascontiguousarray(np.asarray(stamps, np.int64).reshape(-1))
        if T.shape[0] != st.shape[0]:
            raise IcetError(ICET_ERR_BAD_ARG, "poses and stamps differ in length")
        return T, st

    def set_pose(self, slots, poses, stamps):
        """Give occupied slots a pose (4 x 4 float32 each: the physical sensor pose, p_world = R p + t) and an int64 stamp
        (icet_keyframe_store_set_pose).  In stream order with puts and queries; a later put into a slot clears its pose."""
        T, st = self._poses(poses, stamps)
        sl = self._index(slots, T.shape[0])
        self._check(load_library().icet_keyframe_store_set_pose(self._h, T.shape[0], sl.ctypes.data, T.ctypes.data, st.ctypes.data))

    def candidates_device(self, poses, stamps, query, d_cand_ptr, d_x0_base_ptr=None):
        """icet_keyframe_store_candidates_device: the search alone, into device buffers (Q x K int32; Q x K x 6 float32 or None).  Asynchronous."""
        T, st = self._poses(poses, stamps)
        self._check(load_library().icet_keyframe_store_candidates_device(self._h, T.shape[0], T.ctypes.data, st.ctypes.data, C.byref(query), C.c_void_p(d_cand_ptr),
                                                                          C.c_void_p(d_x0_base_ptr) if d_x0_base_ptr else None))

    def candidates(self, poses, stamps, radius, k, min_stamp_gap=0):
        """Place recognition by pose: for every query pose the first ``k`` eligible slots in ascending (d2, slot) order (include/icet_hip.h, CANDIDATES).
        Returns (cand, x0_base): (Q, k) int32 with -1 behind the last, and (Q, k, 6) float32 start poses (zeros for -1)."""
        import torch
        dev = torch.device("cuda", self._ctx.device)
        T, st = self._poses(poses, stamps)
        q = T.shape[0]
        cand = torch.full((q, int(k)), -2, dtype=torch.int32, device=dev)
        x0 = torch.zeros((q, int(k), 6), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        self.candidates_device(T, st, ClosureQuery(float(radius), int(k), int(min_stamp_gap), 1, float("inf"), 0, 0), cand.data_ptr(), x0.data_ptr())
        self._ctx.sync()
        return cand.cpu().numpy(), x0.cpu().numpy()

    def close_device(self, scan2_descs, poses, stamps, params, query, d_closure_ptr, start_offsets=None, d_cand_ptr=None, d_x0_ptr=None, d_out_ptr=None, d_score_ptr=None):
        """icet_keyframe_store_close_device: find, register, score, pick and gate, one record (CLOSURE_DTYPE) per scan.  Asynchronous on the context's stream."""
        T, st = self._poses(poses, stamps)
        q = len(scan2_descs)
        if T.shape[0] != q:
            raise IcetError(ICET_ERR_BAD_ARG, "scans and poses differ in length")
        B = _dev_scans(scan2_descs)
        off = _start_offsets(start_offsets, query)
        self._check(load_library().icet_keyframe_store_close_device(self._h, C.byref(params), q, B, T.ctypes.data, st.ctypes.data, C.byref(query),
                                                                     _data(off), C.c_void_p(d_closure_ptr),
                                                                     _vp(d_cand_ptr), _vp(d_x0_ptr), _vp(d_out_ptr), _vp(d_score_ptr)))

    def find_closures(self, scans, poses, stamps, runlen, radius, k, starts=None, min_stamp_gap=0, max_chi2_per_voxel=float("inf"), min_voxels=0, flags=0):
        """The loop-closure query for host scans (N x 3 each) with their poses and stamps: one dict per scan -- slot (None: no winner), accepted, reg,
        n_candidates, stamp, d2, x0, X, pred_stds, cov, score -- from one icet_keyframe_store_close_device call.  ``starts``: S x 6 offsets added to each
        candidate's start pose (default: one start, no offset)."""
        off = np.zeros((1, 6), np.float32) if starts is None else np.ascontiguousarray(np.asarray(starts, np.float32).reshape(-1, 6))
        query = ClosureQuery(float(radius), int(k), int(min_stamp_gap), off.shape[0], float(max_chi2_per_voxel), int(min_voxels), 0)
        return self._closures(scans, lambda descs, rec: self.close_device(descs, poses, stamps, self._params(runlen, flags), query, rec, off), False, False)

    def _closures(self, scans, call, by_appearance, coarse):
        """Host scans (N x 3 each) staged on the device, ``call(scan2_descs, d_closure_ptr)`` -- one of the close_*_device forms -- and its records as dicts."""
        import torch
        dev = torch.device("cuda", self._ctx.device)
        bufs = [torch.from_numpy(_colmajor(s)).to(dev) for s in scans]
        rec = torch.zeros((len(bufs), CLOSURE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        call([(b.data_ptr(), b.shape[1], b.shape[1]) for b in bufs], rec.data_ptr())
        self._ctx.sync()
        return _closure_dicts(np.frombuffer(rec.cpu().numpy().tobytes(), CLOSURE_DTYPE), by_appearance, coarse)

    # ---- snapshots (include/icet_hip.h "snapshots") ----

    def save(self, path, slots=None):
        """The occupied slots (or the distinct occupied ``slots``) with their poses, stamps, descriptors and grids into the file ``path``
        (icet_keyframe_store_save).  In stream order behind what was enqueued; returns once the file is closed.  A failed save leaves nothing at ``path``."""
        if slots is None:
            self._check(load_library().icet_keyframe_store_save(self._h, os.fsencode(path), 0, None))
            return
        sl = np.ascontiguousarray(np.asarray(slots, np.int32).reshape(-1))
        self._check(load_library().icet_keyframe_store_save(self._h, os.fsencode(path), sl.shape[0], sl.ctypes.data))

    def load(self, path, slot_offset=0):
        """The slots of the file ``path`` into slots ``slot + slot_offset`` of this store, bit for bit (icet_keyframe_store_load): each replaces everything its
        target held, every other slot keeps its bytes.  The file is validated and held against the store first; a refusal touches nothing."""
        self._check(load_library().icet_keyframe_store_load(self._h, os.fsencode(path), int(slot_offset)))

    @staticmethod
    def snapshot_info(path):
        """What the file ``path`` holds, read and validated on the host: dict(num_bins_phi, num_bins_theta, n, thresh, buff, flags, V, entries, highest_slot,
        appearance, coarse, file_bytes, slots, stamps) -- appearance / coarse: the keyword arguments of enable_appearance / enable_coarse, or None."""
        L = load_library()
        info = SnapshotInfo()
        st = L.icet_keyframe_store_snapshot_info(os.fsencode(path), C.byref(info))
        if st != ICET_OK:
            raise IcetError(st, "%s cannot be read or is not a valid keyframe-store snapshot" % path)
        slots = np.zeros(max(info.entries, 1), np.int32); stamps = np.zeros(max(info.entries, 1), np.int64); n = C.c_int32(0)
        st = L.icet_keyframe_store_snapshot_slots(os.fsencode(path), info.entries, slots.ctypes.data, stamps.ctypes.data, C.byref(n))
        if st != ICET_OK or n.value != info.entries:
            raise IcetError(ICET_ERR_BAD_ARG, "%s changed while it was read" % path)
        a, c, p = info.appearance, info.coarse, info.shape
        return dict(num_bins_phi=p.bins_phi, num_bins_theta=p.bins_theta, n=p.n, thresh=p.thresh, buff=p.buff, flags=p.flags, V=info.V, entries=info.entries,
                    highest_slot=info.highest_slot, file_bytes=info.file_bytes, slots=slots[:info.entries], stamps=stamps[:info.entries],
                    appearance=dict(sectors=a.sectors, rings=a.rings, rho_max=a.rho_max, z_lo=a.z_lo, z_hi=a.z_hi) if info.has_appearance else None,
                    coarse=dict(cells=c.cells, cell=c.cell, z_lo=c.z_lo, z_hi=c.z_hi, min_span=c.min_span) if info.has_coarse else None)

    @classmethod
    def from_file(cls, ctx, path, capacity=None):
        """A store of the file's shape on ``ctx`` -- ``capacity`` slots, by default just enough --, appearance and coarse alignment enabled with the saved
        parameters where the file has them, and the file loaded."""
        info = cls.snapshot_info(path)
        need = info["highest_slot"] + 1
        st = cls(ctx, max(1, need) if capacity is None else int(capacity), info["num_bins_phi"], info["num_bins_theta"], info["n"], info["thresh"], info["buff"], info["flags"])
        if info["appearance"] is not None:
            st.enable_appearance(**info["appearance"])
        if info["coarse"] is not None:
            st.enable_coarse(**info["coarse"])
        st.load(path)
        return st

    # ---- loop closure by appearance (include/icet_hip.h "loop closure by appearance") ----

    def enable_appearance(self, sectors=120, rings=20, rho_max=80.0, z_lo=-3.0, z_hi=12.0):
        """Keep a rotation-invariant descriptor (rings x sectors bytes) beside every slot put from now on (icet_keyframe_store_enable_appearance).  Once per
        store; slots put before have no descriptor and are never appearance candidates."""
        ap = AppearanceParams(int(sectors), int(rings), float(rho_max), float(z_lo), float(z_hi), (C.c_int32 * 3)(0, 0, 0))
        self._check(load_library().icet_keyframe_store_enable_appearance(self._h, C.byref(ap)))
        self.appearance = ap

    def describe_device(self, scan_descs, d_desc_ptr, d_weight_ptr, d_rows_ptr=None):
        """icet_keyframe_store_describe_device: the descriptors of device scans into device buffers (n x rings x sectors uint8, n x sectors float32).  Asynchronous."""
        k = len(scan_descs)
        A = _dev_scans(scan_descs)
        self._check(load_library().icet_keyframe_store_describe_device(self._h, k, A, C.c_void_p(d_rows_ptr) if d_rows_ptr else None,
                                                                        C.c_void_p(d_desc_ptr), C.c_void_p(d_weight_ptr)))

    def describe(self, scans):
        """The descriptors of host scans (N x 3 each): ((n, rings, sectors) uint8, (n, sectors) float32)."""
        import torch
        if self.appearance is None:
            raise IcetError(ICET_ERR_BAD_ARG, "appearance is not enabled on this store")
        dev = torch.device("cuda", self._ctx.device)
        a = self.appearance
        bufs = [torch.from_numpy(_colmajor(s)).to(dev) for s in scans]
        D = torch.zeros((max(len(bufs), 1), a.rings, a.sectors), dtype=torch.uint8, device=dev)
        w = torch.zeros((max(len(bufs), 1), a.sectors), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        self.describe_device([(b.data_ptr(), b.shape[1], b.shape[1]) for b in bufs], D.data_ptr(), w.data_ptr())
        self._ctx.sync()
        return D.cpu().numpy()[:len(bufs)], w.cpu().numpy()[:len(bufs)]

    def set_stamp(self, slots, stamps):
        """Give occupied slots an int64 stamp without a pose (icet_keyframe_store_set_stamp); a later put into a slot clears it."""
        st = np.ascontiguousarray(np.asarray(stamps, np.int64).reshape(-1))
        sl = self._index(slots, st.shape[0])
        self._check(load_library().icet_keyframe_store_set_stamp(self._h, st.shape[0], sl.ctypes.data, st.ctypes.data))

    @staticmethod
    def _stamps(stamps, q):
        if stamps is None:
            return None
        st = np.ascontiguousarray(np.asarray(stamps, np.int64).reshape(-1))
        if st.shape[0] != q:
            raise IcetError(ICET_ERR_BAD_ARG, "scans and stamps differ in length")
        return st

    def candidates_appearance_device(self, scan2_descs, stamps, query, d_cand_ptr, d_dist_ptr=None, d_shift_ptr=None, d_x0_base_ptr=None):
        """icet_keyframe_store_candidates_appearance_device: the appearance search alone, into device buffers.  ``query.radius`` is read as max_distance."""
        q = len(scan2_descs)
        st = self._stamps(stamps, q)
        B = _dev_scans(scan2_descs)
        self._check(load_library().icet_keyframe_store_candidates_appearance_device(self._h, q, B, _data(st), C.byref(query),
                                                                                     _vp(d_cand_ptr), _vp(d_dist_ptr), _vp(d_shift_ptr), _vp(d_x0_base_ptr)))

    def candidates_by_appearance(self, scans, k, max_distance, stamps=None, min_stamp_gap=0):
        """Place recognition without poses: for every host scan (N x 3) the first ``k`` eligible slots in ascending (distance, slot) order.  Returns
        (cand, dist, shift, x0_base): (Q, k) int32 with -1 behind the last, (Q, k) float32 (+inf), (Q, k) int32 (-1), (Q, k, 6) float32 (zeros)."""
        import torch
        dev = torch.device("cuda", self._ctx.device)
        bufs = [torch.from_numpy(_colmajor(s)).to(dev) for s in scans]
        q = len(bufs)
        cand = torch.full((q, int(k)), -2, dtype=torch.int32, device=dev)
        dist = torch.zeros((q, int(k)), dtype=torch.float32, device=dev)
        shift = torch.full((q, int(k)), -2, dtype=torch.int32, device=dev)
        x0 = torch.zeros((q, int(k), 6), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        self.candidates_appearance_device([(b.data_ptr(), b.shape[1], b.shape[1]) for b in bufs], stamps,
                                          ClosureQuery(float(max_distance), int(k), int(min_stamp_gap), 1, float("inf"), 0, 0),
                                          cand.data_ptr(), dist.data_ptr(), shift.data_ptr(), x0.data_ptr())
        self._ctx.sync()
        return cand.cpu().numpy(), dist.cpu().numpy(), shift.cpu().numpy(), x0.cpu().numpy()

    def close_appearance_device(self, scan2_descs, stamps, params, query, d_closure_ptr, start_offsets=None, d_cand_ptr=None, d_x0_ptr=None, d_out_ptr=None, d_score_ptr=None):
        """icet_keyframe_store_close_appearance_device: close_device without poses -- the candidates come from the appearance search and the yaw of each
        start pose from the best column shift; ``query.radius`` is read as max_distance.  One record (CLOSURE_DTYPE; d2 = distance, reserved0 = shift) per scan."""
        q = len(scan2_descs)
        st = self._stamps(stamps, q)
        B = _dev_scans(scan2_descs)
        off = _start_offsets(start_offsets, query)
        self._check(load_library().icet_keyframe_store_close_appearance_device(self._h, C.byref(params), q, B, _data(st), C.byref(query),
                                                                                _data(off), C.c_void_p(d_closure_ptr),
                                                                                _vp(d_cand_ptr), _vp(d_x0_ptr), _vp(d_out_ptr), _vp(d_score_ptr)))

    def find_closures_by_appearance(self, scans, runlen, k, starts=LATTICE_STARTS, max_distance=float("inf"), stamps=None, min_stamp_gap=0,
                                    max_chi2_per_voxel=float("inf"), min_voxels=0, flags=0):
        """find_closures without poses, for host scans (N x 3 each): one dict per scan -- slot (None: no winner), accepted, reg, n_candidates, stamp,
        distance, shift, x0, X, pred_stds, cov, score -- from one icet_keyframe_store_close_appearance_device call.  ``starts``: S x 6 offsets added to
        (0, 0, 0, 0, 0, yaw of the shift); the default is the 3 x 3 lattice of +-0.3 m, because the search finds the yaw and not the translation."""
        off = np.ascontiguousarray(np.asarray(starts, np.float32).reshape(-1, 6))
        query = ClosureQuery(float(max_distance), int(k), int(min_stamp_gap), off.shape[0], float(max_chi2_per_voxel), int(min_voxels), 0)
        return self._closures(scans, lambda descs, rec: self.close_appearance_device(descs, stamps, self._params(runlen, flags), query, rec, off), True, False)

    # ---- coarse alignment (include/icet_hip.h "coarse alignment") ----

    def enable_coarse(self, cells=256, cell=0.25, z_lo=-3.0, z_hi=12.0, min_span=0.5):
        """Keep a bird's-eye bit grid (cells x cells bits of vertical structure) beside every slot put from now on (icet_keyframe_store_enable_coarse).  Once per
        store; slots put before have no grid and the search reports found = 0 for them."""
        cp = CoarseParams(int(cells), float(cell), float(z_lo), float(z_hi), float(min_span), (C.c_int32 * 3)(0, 0, 0))
        self._check(load_library().icet_keyframe_store_enable_coarse(self._h, C.byref(cp)))
        self.coarse = cp

    @staticmethod
    def coarse_search(window=12, n_yaw=1, yaw_step=np.pi / 120, half_turn=True, min_score=1):
        """An icet_coarse_search record; the defaults suit candidates by appearance at 120 sectors (yaw_step = pi / sectors)."""
        return CoarseSearch(int(window), int(n_yaw), float(yaw_step), int(bool(half_turn)), int(min_score), (C.c_int32 * 3)(0, 0, 0))

    def coarse_grid_device(self, scan_descs, d_grid_ptr, d_rows_ptr=None):
        """icet_keyframe_store_coarse_grid_device: the grids of device scans into a device buffer (n x cells x cells / 32 uint32).  Asynchronous."""
        k = len(scan_descs)
        A = _dev_scans(scan_descs)
        self._check(load_library().icet_keyframe_store_coarse_grid_device(self._h, k, A, C.c_void_p(d_rows_ptr) if d_rows_ptr else None, C.c_void_p(d_grid_ptr)))

    def coarse_grid(self, scans):
        """The grids of host scans (N x 3 each): (n, cells, cells / 32) uint32."""
        import torch
        if self.coarse is None:
            raise IcetError(ICET_ERR_BAD_ARG, "coarse alignment is not enabled on this store")
        dev = torch.device("cuda", self._ctx.device)
        G = self.coarse.cells
        bufs = [torch.from_numpy(_colmajor(s)).to(dev) for s in scans]
        g = torch.zeros((max(len(bufs), 1), G, G // 32), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.coarse_grid_device([(b.data_ptr(), b.shape[1], b.shape[1]) for b in bufs], g.data_ptr())
        self._ctx.sync()
        return g.cpu().numpy().view(np.uint32)[:len(bufs)]

    def coarse_align_device(self, scan2_descs, k, d_cand_ptr, d_x0_base_ptr, search, d_x0_out_ptr=None, d_match_ptr=None, d_rows_ptr=None):
        """icet_keyframe_store_coarse_align_device: the search alone for Q x k candidates (device buffers as either candidates call writes them).  Asynchronous."""
        q = len(scan2_descs)
        B = _dev_scans(scan2_descs)
        self._check(load_library().icet_keyframe_store_coarse_align_device(self._h, q, B, _vp(d_rows_ptr), int(k), _vp(d_cand_ptr), _vp(d_x0_base_ptr), C.byref(search),
                                                                            _vp(d_x0_out_ptr), _vp(d_match_ptr)))

    def coarse_align(self, scans, cand, x0_base, window=12, n_yaw=1, yaw_step=np.pi / 120, half_turn=True, min_score=1):
        """The coarse search for host scans (N x 3 each): ``cand`` (Q, k) slots (-1: none) and ``x0_base`` (Q, k, 6) base starts, e.g. from candidates() or
        candidates_by_appearance().  Returns (x0, match): (Q, k, 6) float32 start poses and (Q, k) records of COARSE_MATCH_DTYPE."""
        import torch
        dev = torch.device("cuda", self._ctx.device)
        cand = np.ascontiguousarray(np.asarray(cand, np.int32))
        q, k = cand.shape
        base = np.ascontiguousarray(np.asarray(x0_base, np.float32).reshape(q, k, 6))
        bufs = [torch.from_numpy(_colmajor(s)).to(dev) for s in scans]
        if len(bufs) != q:
            raise IcetError(ICET_ERR_BAD_ARG, "scans and cand differ in length")
        dc = torch.from_numpy(cand).to(dev); db = torch.from_numpy(base).to(dev)
        x0 = torch.zeros((q, k, 6), dtype=torch.float32, device=dev)
        m = torch.zeros((q, k, COARSE_MATCH_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        self.coarse_align_device([(b.data_ptr(), b.shape[1], b.shape[1]) for b in bufs], k, dc.data_ptr(), db.data_ptr(),
                                 self.coarse_search(window, n_yaw, yaw_step, half_turn, min_score), x0.data_ptr(), m.data_ptr())
        self._ctx.sync()
        return x0.cpu().numpy(), np.frombuffer(m.cpu().numpy().tobytes(), COARSE_MATCH_DTYPE).reshape(q, k).copy()

    def close_coarse_device(self, scan2_descs, poses, stamps, params, query, search, d_closure_ptr, start_offsets=None, d_cand_ptr=None, d_x0_ptr=None, d_out_ptr=None,
                            d_score_ptr=None, d_match_ptr=None):
        """icet_keyframe_store_close_coarse_device: close_device (``poses`` given) or close_appearance_device (``poses`` None) with the coarse alignment of every
        candidate's base start in between.  One record (CLOSURE_DTYPE; reserved1 = coarse score, h | (a + 32) << 8 | (b + 32) << 16) per scan."""
        q = len(scan2_descs)
        T = None
        if poses is not None:
            T, st = self._poses(poses, stamps)
            if T.shape[0] != q:
                raise IcetError(ICET_ERR_BAD_ARG, "scans and poses differ in length")
        else:
            st = self._stamps(stamps, q)
        B = _dev_scans(scan2_descs)
        off = _start_offsets(start_offsets, query)
        self._check(load_library().icet_keyframe_store_close_coarse_device(self._h, C.byref(params), q, B, _data(T),
                                                                            _data(st), C.byref(query), C.byref(search),
                                                                            _data(off), C.c_void_p(d_closure_ptr),
                                                                            _vp(d_cand_ptr), _vp(d_x0_ptr), _vp(d_out_ptr), _vp(d_score_ptr), _vp(d_match_ptr)))

    def find_closures_coarse(self, scans, runlen, k, poses=None, stamps=None, starts=None, radius=float("inf"), min_stamp_gap=0, window=12, n_yaw=1, yaw_step=None,
                             half_turn=True, min_score=1, max_chi2_per_voxel=float("inf"), min_voxels=0, flags=0):
        """find_closures (``poses`` given; ``radius`` in metres) or find_closures_by_appearance (``poses`` None; ``radius`` is max_distance) with the coarse alignment
        of every candidate's start, for host scans (N x 3 each): their dicts plus ``coarse`` = dict(score, a, b, h) of the winner.  ``starts``: S x 6 offsets
        added to the coarse start (default: one start, no offset).  ``yaw_step`` defaults to pi / sectors of the appearance search, pi / 120 without one."""
        off = np.zeros((1, 6), np.float32) if starts is None else np.ascontiguousarray(np.asarray(starts, np.float32).reshape(-1, 6))
        if yaw_step is None:
            yaw_step = np.pi / (self.appearance.sectors if self.appearance is not None else 120)
        query = ClosureQuery(float(radius), int(k), int(min_stamp_gap), off.shape[0], float(max_chi2_per_voxel), int(min_voxels), 0)
        search = self.coarse_search(window, n_yaw, yaw_step, half_turn, min_score)
        return self._closures(scans, lambda descs, rec: self.close_coarse_device(descs, poses, stamps, self._params(runlen, flags), query, search, rec, off),
                              poses is None, True)

    def best_match(self, scan2, slot_index, x0, runlen, flags=0):
        """The loop-closure check: registration r = host scan2 (N x 3) against slot slot_index[r] from x0[r]; all of them one group, scored and
        reduced on the device (icet_select_best_device).  Returns dict(best, slot, X, pred_stds, cov, score, X_all) like Context.solve_multistart:
        ``best`` the winning registration (-1: none has a contributing voxel; slot, X, pred_stds, cov are then None), ``slot`` its slot."""
        import torch
        dev = torch.device("cuda", self._ctx.device)
        idx = np.ascontiguousarray(np.asarray(slot_index, np.int32).reshape(-1))
        k = idx.shape[0]
        x = np.ascontiguousarray(np.asarray(x0, np.float32).reshape(k, 6))
        s2 = torch.from_numpy(_colmajor(scan2)).to(dev)
        xd = torch.from_numpy(x).to(dev)
        out = torch.zeros((k, 48), dtype=torch.float32, device=dev)
        sc = torch.zeros((k, 8), dtype=torch.int32, device=dev)
        best = torch.full((1,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.register_scored_device(idx, [(s2.data_ptr(), s2.shape[1], s2.shape[1])] * k, self._params(runlen, flags), out.data_ptr(), sc.data_ptr(), xd.data_ptr())
        self._ctx.select_best_device(np.zeros(k, np.int32), 1, sc.data_ptr(), best.data_ptr())
        self._ctx.sync()
        score = scores_as_dict(np.frombuffer(sc.cpu().numpy().tobytes(), SCORE_DTYPE))
        o = out.cpu().numpy()
        b = int(best.cpu().numpy()[0])
        res = dict(best=b, score=score, X_all=o[:, :6].copy())
        if b < 0:
            res.update(slot=None, X=None, pred_stds=None, cov=None)
        else:
            res.update(slot=int(idx[b]), X=o[b, :6].copy(), pred_stds=o[b, 6:12].copy(), cov=o[b, 12:48].reshape(6, 6).copy())
        return res


class VoxelMap:
    """``icet_voxel_map`` (include/icet_hip.h): scans at 4 x 4 poses fused into one centroid and one count per occupied cell on ``ctx``'s
    device.  ``remove`` undoes an ``add`` at the same pose exactly, so a scan can be moved to a corrected pose; ``extract`` gives the cells sorted by key as a
    scan.  The map borrows ``ctx`` (closed before it)."""

    def __init__(self, ctx, cell=0.1, min_range=0.0, max_range=0.0, table_log2=22, shape=False):
        self._ctx = ctx
        self.shape = False
        self.params = MapParams(float(cell), float(min_range), float(max_range), int(table_log2), 0)
        h = C.c_void_p()
        st = load_library().icet_voxel_map_create(ctx._h, C.byref(self.params), C.byref(h))
        if st != ICET_OK:
            raise IcetError(st, "icet_voxel_map_create: " + load_library().icet_last_error(ctx._h).decode())
        self._h = h
        import weakref
        if not hasattr(ctx, "_nodes"):
            ctx._nodes = []
        ctx._nodes.append(weakref.ref(self))
        if shape:
            try:
                self.enable_shape()
            except Exception:
                self.close()
                raise

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self._ctx, "_h", None):               # (a context finalised first took the device with it: see KeyframeStore.close)
                load_library().icet_voxel_map_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != ICET_OK:
            raise IcetError(st, load_library().icet_voxel_map_last_error(self._h).decode())

    def _add_device(self, descs, poses, sign):
        A = _dev_scans(descs)
        if isinstance(poses, np.ndarray) or not hasattr(poses, "data_ptr"):
            T = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 16))
            if T.shape[0] != len(descs):
                raise IcetError(ICET_ERR_BAD_ARG, "one 4 x 4 pose per scan")
            self._check(load_library().icet_voxel_map_add_device(self._h, len(descs), A, T.ctypes.data, int(sign)))
            return
        import torch
        if not (poses.is_cuda and poses.dtype == torch.float32 and poses.is_contiguous()) or poses.numel() != 16 * len(descs):
            raise IcetError(ICET_ERR_BAD_ARG, "device poses must be a contiguous float32 CUDA tensor of one 4 x 4 pose per scan")
        torch.cuda.current_stream(poses.device).synchronize()          # the context's stream is its own: the tensor must be complete
        self._check(load_library().icet_voxel_map_add_posed_device(self._h, len(descs), A, _vp(poses.data_ptr()), int(sign)))

    def add_device(self, descs, poses):
        """Add the scans (device_ptr, n, ld) at ``poses``: an n x 4 x 4 NumPy array (icet_voxel_map_add_device) or a float32 CUDA tensor
        (icet_voxel_map_add_posed_device).  Asynchronous on the context's stream."""
        self._add_device(descs, poses, 1)

    def remove_device(self, descs, poses):
        """Remove the scans at the poses they were added at (sign -1)."""
        self._add_device(descs, poses, -1)

    def _add_host(self, scans, poses, sign):
        import torch
        dev = torch.device("cuda", self._ctx.device)
        bufs = [torch.from_numpy(_colmajor(s)).to(dev) for s in scans]
        torch.cuda.synchronize(dev)
        self._add_device([(b.data_ptr(), b.shape[1], b.shape[1]) for b in bufs], poses, sign)
        self._ctx.sync()

    def add(self, scans, poses):
        """add_device for host N x 3 arrays: staged on the device; returns once the add has run."""
        self._add_host(scans, poses, 1)

    def remove(self, scans, poses):
        self._add_host(scans, poses, -1)

    def clear(self):
        self._check(load_library().icet_voxel_map_clear(self._h))

    def stats(self, min_points=1):
        """The running totals since the last clear and the cells as they are now (MapStats.as_dict()).  Synchronises."""
        s = MapStats()
        self._check(load_library().icet_voxel_map_stats(self._h, int(min_points), C.byref(s)))
        return s.as_dict()

    def extract_device(self, d_xyz_ptr, ld, cap_rows, min_points=1, d_count_ptr=None, d_key_ptr=None):
        """The cells with count >= max(1, min_points), sorted by key, into device buffers: d_xyz N x 3 column-major float32 (leading dimension ld), optional
        int64 counts and uint64 keys.  Returns the stats; cells_out rows exist, min(cells_out, cap_rows) were written.  Synchronises."""
        s = MapStats()
        self._check(load_library().icet_voxel_map_extract_device(self._h, int(min_points), _vp(d_xyz_ptr), int(ld), int(cap_rows), _vp(d_count_ptr), _vp(d_key_ptr),
                                                                 C.byref(s)))
        return s.as_dict()

    def extract(self, min_points=1, cap_rows=None):
        """The map on the host: dict(xyz (n, 3) float32, count (n,) int64, key (n,) uint64, stats).  cap_rows: at most so many rows (the lowest keys)."""
        cap = self.stats(min_points)["cells_out"] if cap_rows is None else int(cap_rows)
        xyz = np.zeros((3, max(cap, 1)), np.float32); cnt = np.zeros(max(cap, 1), np.int64); key = np.zeros(max(cap, 1), np.uint64)
        s = MapStats()
        self._check(load_library().icet_voxel_map_extract(self._h, int(min_points), xyz.ctypes.data, max(cap, 1), cap, cnt.ctypes.data, key.ctypes.data, C.byref(s)))
        n = min(cap, s.cells_out)
        return dict(xyz=np.ascontiguousarray(xyz[:, :n].T), count=cnt[:n].copy(), key=key[:n].copy(), stats=s.as_dict())

    def enable_shape(self):
        """Carry nine integer moment words per cell from now on (icet_voxel_map_enable_shape), so that extract_shape gives a covariance,
        eigenvalues and a normal per cell.  Only on a map that has read no row since it was created or last cleared; does nothing on a shaped map."""
        self._check(load_library().icet_voxel_map_enable_shape(self._h))
        self.shape = True

    def save(self, path):
        """The map's cells and running totals into the file ``path`` (icet_voxel_map_save): every claimed entry with a non-zero word, by
        ascending key, so the bytes are a function of the map's contents alone.  In stream order behind what was enqueued; returns once the file is closed.  A
        failed save leaves nothing at ``path``.  The map is not changed."""
        self._check(load_library().icet_voxel_map_save(self._h, os.fsencode(path)))

    def load(self, path, sign=1):
        """Add (``sign`` 1) or subtract (-1) the cells and totals of the file ``path`` (icet_voxel_map_load).  The file is validated and held against the map
        first -- the same cell, no plain file into a shaped map, room for its new keys --; a refusal touches nothing.  Synchronises."""
        self._check(load_library().icet_voxel_map_load(self._h, os.fsencode(path), int(sign)))

    @staticmethod
    def snapshot_info(path):
        """What the file ``path`` holds, read and validated on the host: dict(cell, min_range, max_range, shaped, words_per_entry, entries, the five totals,
        file_bytes, payload_checksum)."""
        info = MapSnapshotInfo()
        st = load_library().icet_voxel_map_snapshot_info(os.fsencode(path), C.byref(info))
        if st != ICET_OK:
            raise IcetError(st, "%s cannot be read or is not a valid voxel-map snapshot" % path)
        d = {n: getattr(info, n) for n, _ in info._fields_ if not n.startswith("reserved")}
        d["shaped"] = bool(d["shaped"])
        return d

    @classmethod
    def from_file(cls, ctx, path, table_log2=None):
        """A new map on ``ctx`` with the file's cell, ranges and shape, holding its contents.  ``table_log2``: by default the smallest table that the file's
        entries fill at most half, never below 10."""
        info = cls.snapshot_info(path)
        if table_log2 is None:
            table_log2 = max(10, (2 * max(int(info["entries"]), 1) - 1).bit_length())
        m = cls(ctx, cell=info["cell"], min_range=info["min_range"], max_range=info["max_range"], table_log2=table_log2, shape=info["shaped"])
        try:
            m.load(path)
        except Exception:
            m.close()
            raise
        return m

    def merge(self, other, sign=1):
        """Add (``sign`` 1) or subtract (-1) the cells and totals of ``other``, a map of the same cell on the same context (icet_voxel_map_merge_device): load's
        rules with the source in device memory.  ``other`` is only read."""
        if not isinstance(other, VoxelMap) or not getattr(other, "_h", None):
            raise IcetError(ICET_ERR_BAD_ARG, "merge takes an open VoxelMap")
        self._check(load_library().icet_voxel_map_merge_device(self._h, other._h, int(sign)))

    def grown(self, table_log2):
        """A new map with a table of 2^table_log2 entries and this map's parameters, shape, contents and totals (through ``merge``): the answer to
        VOXEL_MAP_TABLE_FULL.  Entries that a remove emptied are not carried over.  This map is only read."""
        m = VoxelMap(self._ctx, cell=self.params.cell, min_range=self.params.min_range, max_range=self.params.max_range, table_log2=table_log2, shape=self.shape)
        try:
            m.merge(self)
        except Exception:
            m.close()
            raise
        return m

    def extract_shape_device(self, d_xyz_ptr, ld, cap_rows, min_points=1, d_count_ptr=None, d_key_ptr=None, d_cov_ptr=None, d_normal_ptr=None, d_evals_ptr=None,
                             d_moments_ptr=None, shape_ld=None):
        """extract_device's rows, and per row the shape columns into device buffers, each column-major over ``shape_ld`` (default ld): d_cov 6 float32 columns (xx,
        xy, xz, yy, yz, zz), d_normal 3, d_evals 3 (ascending), d_moments 9 uint64 columns (the raw words); any may be left out.  Returns the stats.  Synchronises."""
        s = MapStats()
        sh = MapShape(*[int(p) if p else None for p in (d_cov_ptr, d_normal_ptr, d_evals_ptr, d_moments_ptr)], int(ld if shape_ld is None else shape_ld), 0, 0)
        self._check(load_library().icet_voxel_map_extract_shape_device(self._h, int(min_points), _vp(d_xyz_ptr), int(ld), int(cap_rows), _vp(d_count_ptr), _vp(d_key_ptr),
                                                                       C.byref(sh), C.byref(s)))
        return s.as_dict()

    def extract_shape(self, min_points=1, cap_rows=None, moments=False):
        """extract's dict, and cov (n, 6) float32, normal (n, 3) float32, evals (n, 3) float32 ascending; ``moments``: also the nine raw words, (n, 9) uint64."""
        cap = self.stats(min_points)["cells_out"] if cap_rows is None else int(cap_rows)
        ld = max(cap, 1)
        xyz = np.zeros((3, ld), np.float32); cnt = np.zeros(ld, np.int64); key = np.zeros(ld, np.uint64)
        cov = np.zeros((6, ld), np.float32); nrm = np.zeros((3, ld), np.float32); ev = np.zeros((3, ld), np.float32)
        mom = np.zeros((9, ld), np.uint64) if moments else None
        sh = MapShape(cov.ctypes.data, nrm.ctypes.data, ev.ctypes.data, mom.ctypes.data if moments else None, ld, 0, 0)
        s = MapStats()
        self._check(load_library().icet_voxel_map_extract_shape(self._h, int(min_points), xyz.ctypes.data, ld, cap, cnt.ctypes.data, key.ctypes.data, C.byref(sh), C.byref(s)))
        n = min(cap, s.cells_out)
        res = dict(xyz=np.ascontiguousarray(xyz[:, :n].T), count=cnt[:n].copy(), key=key[:n].copy(), cov=np.ascontiguousarray(cov[:, :n].T),
                   normal=np.ascontiguousarray(nrm[:, :n].T), evals=np.ascontiguousarray(ev[:, :n].T), stats=s.as_dict())
        if moments:
            res["moments"] = np.ascontiguousarray(mom[:, :n].T)
        return res

    def index(self):
        """Rebuild the sorted index the queries read, if the map changed since the last one (icet_voxel_map_index).  Returns the stats at min_points 1 as the
        build saw them.  Synchronises when it builds; does nothing otherwise."""
        s = MapStats()
        self._check(load_library().icet_voxel_map_index(self._h, C.byref(s)))
        return s.as_dict()

    def evidence_device(self, descs, poses, max_range, margin=None, min_range=0.0, image_log2=8, window=1, min_miss=2, agree_factor=1, stats=True):
        """The visibility evidence of the map's cells from the scans (device_ptr, n, ld) at ``poses`` (an n x 4 x 4 NumPy array: icet_voxel_map_evidence_device; a
        float32 CUDA tensor: icet_voxel_map_evidence_posed_device): per cell of the index how many scans measured something further away through it (miss) and
        how many measured it (agree), and the decision transient = miss >= max(1, min_miss) and miss > agree_factor * agree.  margin None: three cells.  The map
        keeps the evidence (evidence_fetch, ``static=True`` of the queries) until the next add, remove or clear.  Returns the stats as a dict and synchronises;
        ``stats=False``: returns None, asynchronous on the context's stream unless the index is stale."""
        A = _dev_scans(descs)
        mg = 3.0 * float(self.params.cell) if margin is None else float(margin)
        e = MapEvidence(float(min_range), float(max_range), mg, int(image_log2), int(window), int(min_miss), int(agree_factor), 0)
        s = MapEvidenceStats() if stats else None
        L = load_library()
        if isinstance(poses, np.ndarray) or not hasattr(poses, "data_ptr"):
            T = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 16))
            if T.shape[0] != len(descs):
                raise IcetError(ICET_ERR_BAD_ARG, "one 4 x 4 pose per scan")
            self._check(L.icet_voxel_map_evidence_device(self._h, len(descs), A, T.ctypes.data if len(descs) else None, C.byref(e), C.byref(s) if stats else None))
        else:
            import torch
            if not (poses.is_cuda and poses.dtype == torch.float32 and poses.is_contiguous()) or poses.numel() != 16 * len(descs):
                raise IcetError(ICET_ERR_BAD_ARG, "device poses must be a contiguous float32 CUDA tensor of one 4 x 4 pose per scan")
            torch.cuda.current_stream(poses.device).synchronize()      # the context's stream is its own: the tensor must be complete
            self._check(L.icet_voxel_map_evidence_posed_device(self._h, len(descs), A, _vp(poses.data_ptr()), C.byref(e), C.byref(s) if stats else None))
        return s.as_dict() if stats else None

    def evidence_fetch_device(self, cap, d_miss_ptr=None, d_agree_ptr=None, d_transient_ptr=None):
        """Copy the evidence the map holds into device arrays of ``cap`` entries (int32, int32, uint8; any may be left out), in index order, on the context's
        stream (icet_voxel_map_evidence_fetch_device).  Refused when there is no current evidence or cap is below the cells of the index.  Returns the rows."""
        rows = C.c_int64(0)
        self._check(load_library().icet_voxel_map_evidence_fetch_device(self._h, _vp(d_miss_ptr), _vp(d_agree_ptr), _vp(d_transient_ptr), int(cap), C.byref(rows)))
        return int(rows.value)

    def evidence_fetch(self):
        """The evidence the map holds, on the host: dict(miss (n,) int32, agree (n,) int32, transient (n,) uint8, key (n,) uint64), in index order."""
        import torch
        dev = torch.device("cuda", self._ctx.device)
        n = int(self.index()["cells_out"])
        miss = torch.zeros(max(n, 1), dtype=torch.int32, device=dev); agree = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        tr = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        rows = self.evidence_fetch_device(n, miss.data_ptr(), agree.data_ptr(), tr.data_ptr())
        self._ctx.sync()
        key = self.extract(1)["key"]                                  # the index order is extract's at min_points 1
        return dict(miss=miss[:rows].cpu().numpy(), agree=agree[:rows].cpu().numpy(), transient=tr[:rows].cpu().numpy(), key=key)

    def evidence(self, scans, poses, max_range, margin=None, min_range=0.0, image_log2=8, window=1, min_miss=2, agree_factor=1):
        """evidence_device for host N x 3 arrays, and the fetch: dict(miss, agree, transient, key, stats)."""
        import torch
        dev = torch.device("cuda", self._ctx.device)
        bufs = [torch.from_numpy(_colmajor(s)).to(dev) for s in scans]
        torch.cuda.synchronize(dev)
        st = self.evidence_device([(b.data_ptr(), b.shape[1], b.shape[1]) for b in bufs], poses, max_range, margin, min_range, image_log2, window, min_miss, agree_factor)
        res = self.evidence_fetch()
        res["stats"] = st
        return res

    def register_device(self, descs, poses, d_records_ptr, params=None, **kw):
        """Register the scans (device_ptr, n, ld) against the map's Gaussians from the start ``poses``: a Q x 4 x 4 NumPy array
        (icet_voxel_map_register_device) or a float32 CUDA tensor (icet_voxel_map_register_posed_device; ``register_posed_device`` is this call with a tensor).
        ``d_records_ptr``: Q records of MAP_REGISTRATION_DTYPE on the device.  ``params``: a MapRegisterParams, or keywords over MAP_REGISTER_DEFAULTS; neither:
        NULL, the library's defaults.  Several queries may name one scan.  Asynchronous on the context's stream."""
        A = _dev_scans(descs)
        P = params if params is not None else (map_register_params(**kw) if kw else None)
        pp = C.byref(P) if P is not None else None
        L = load_library()
        if isinstance(poses, np.ndarray) or not hasattr(poses, "data_ptr"):
            T = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 16))
            if T.shape[0] != len(descs):
                raise IcetError(ICET_ERR_BAD_ARG, "one 4 x 4 pose per scan")
            self._check(L.icet_voxel_map_register_device(self._h, len(descs), A, T.ctypes.data if len(descs) else None, pp, _vp(d_records_ptr)))
            return
        import torch
        if not (poses.is_cuda and poses.dtype == torch.float32 and poses.is_contiguous()) or poses.numel() != 16 * len(descs):
            raise IcetError(ICET_ERR_BAD_ARG, "device poses must be a contiguous float32 CUDA tensor of one 4 x 4 pose per scan")
        torch.cuda.current_stream(poses.device).synchronize()          # the context's stream is its own: the tensor must be complete
        self._check(L.icet_voxel_map_register_posed_device(self._h, len(descs), A, _vp(poses.data_ptr()), pp, _vp(d_records_ptr)))

    def register_posed_device(self, descs, d_poses, d_records_ptr, params=None, **kw):
        """register_device with the start poses in a float32 CUDA tensor (icet_voxel_map_register_posed_device)."""
        if not hasattr(d_poses, "data_ptr"):
            raise IcetError(ICET_ERR_BAD_ARG, "register_posed_device takes a CUDA tensor of poses")
        self.register_device(descs, d_poses, d_records_ptr, params, **kw)

    def register_records(self, descs, poses, params=None, **kw):
        """register_device into a buffer of its own; synchronises; the records as a NumPy array of MAP_REGISTRATION_DTYPE."""
        import torch
        dev = torch.device("cuda", self._ctx.device)
        out = torch.zeros(max(len(descs), 1) * MAP_REGISTRATION_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        self.register_device(descs, poses, out.data_ptr(), params, **kw)
        self._ctx.sync()
        return out.cpu().numpy().view(MAP_REGISTRATION_DTYPE)[:len(descs)].copy()

    def register(self, scans, poses, scan_of=None, **params):
        """register_device for host N x 3 arrays: staged on the device, synchronises, one dict per pose -- pose (4, 4) float32, info (21,), g (6,), cost,
        cost_start, lambda, rows_scored, rows_matched, iterations, accepted, status.  ``scan_of``: per pose the index of its scan (default: pose k takes scan k),
        so that several start poses share one staged scan."""
        import torch
        dev = torch.device("cuda", self._ctx.device)
        bufs = [torch.from_numpy(_colmajor(s)).to(dev) for s in scans]
        torch.cuda.synchronize(dev)
        T = np.asarray(poses, np.float32).reshape(-1, 16)
        of = list(range(T.shape[0])) if scan_of is None else [int(k) for k in scan_of]
        descs = [(bufs[k].data_ptr(), bufs[k].shape[1], bufs[k].shape[1]) for k in of]
        recs = self.register_records(descs, T, **params)
        res = []
        for r in recs:
            d = {n: (r[n].copy() if r[n].shape else r[n].item()) for n in MAP_REGISTRATION_DTYPE.names if n != "reserved"}
            d["pose"] = d["pose"].reshape(4, 4)
            res.append(d)
        return res

    def score(self, scans, poses, scan_of=None, **params):
        """The cost, gradient and information of the given poses against the map, without a step: ``register`` with max_iters = 0."""
        params["max_iters"] = 0
        return self.register(scans, poses, scan_of, **params)

    def register_terms(self, scan, pose, **params):
        """icet_debug_voxel_map_register_terms for a host N x 3 array: one record of MAP_REGISTER_TERM_DTYPE per row at ``pose``."""
        import torch
        dev = torch.device("cuda", self._ctx.device)
        buf = torch.from_numpy(_colmajor(scan)).to(dev)
        n = buf.shape[1]
        out = torch.zeros(max(n, 1) * MAP_REGISTER_TERM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        self.register_terms_device((buf.data_ptr(), n, n), pose, out.data_ptr(), **params)
        self._ctx.sync()
        return out.cpu().numpy().view(MAP_REGISTER_TERM_DTYPE)[:n].copy()

    def register_terms_device(self, desc, pose, d_terms_ptr, params=None, **kw):
        """One record per row of the scan (device_ptr, n, ld) at the HOST pose into d_terms (device, n records of MAP_REGISTER_TERM_DTYPE).  Asynchronous."""
        A = _dev_scans([desc])
        P = params if params is not None else (map_register_params(**kw) if kw else None)
        T = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(16))
        self._check(load_library().icet_debug_voxel_map_register_terms(self._h, A, T.ctypes.data, C.byref(P) if P is not None else None, _vp(d_terms_ptr)))

    def query_device(self, poses, outs, d_rows_ptr, min_range=0.0, max_range=0.0, min_points=1, world=False, d_total_ptr=None, d_status_ptr=None, static=False):
        """For each pose the cells of the map within (min_range, max_range] of it, in the pose's own frame (``world``: in the map's), in key order, into device
        buffers.  ``poses``: a Q x 4 x 4 NumPy array (icet_voxel_map_query_device) or a float32 CUDA tensor (icet_voxel_map_query_posed_device); ``outs``: one
        (d_xyz_ptr, ld, cap_rows, d_count_ptr, d_key_ptr) per pose (a MapSubmap each; None for a pointer left out); d_rows / d_total / d_status: device int32
        arrays of Q entries.  ``static``: the cells the current evidence calls transient take no part (refused without current evidence).  Asynchronous on the
        context's stream unless the index is stale."""
        q = MapQuery(float(min_range), float(max_range), int(min_points), (VOXEL_MAP_QUERY_WORLD if world else 0) | (VOXEL_MAP_QUERY_STATIC if static else 0))
        O = (MapSubmap * max(len(outs), 1))(*[MapSubmap(int(o[0]) if o[0] else None, int(o[1]), int(o[2]), int(o[3]) if len(o) > 3 and o[3] else None,
                                                         int(o[4]) if len(o) > 4 and o[4] else None) for o in outs])
        L = load_library()
        if isinstance(poses, np.ndarray) or not hasattr(poses, "data_ptr"):
            T = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 16))
            if T.shape[0] != len(outs):
                raise IcetError(ICET_ERR_BAD_ARG, "one sub-map per 4 x 4 pose")
            self._check(L.icet_voxel_map_query_device(self._h, len(outs), T.ctypes.data, C.byref(q), O, _vp(d_rows_ptr), _vp(d_total_ptr), _vp(d_status_ptr)))
            return
        import torch
        if not (poses.is_cuda and poses.dtype == torch.float32 and poses.is_contiguous()) or poses.numel() != 16 * len(outs):
            raise IcetError(ICET_ERR_BAD_ARG, "device poses must be a contiguous float32 CUDA tensor of one 4 x 4 pose per sub-map")
        torch.cuda.current_stream(poses.device).synchronize()          # the context's stream is its own: the tensor must be complete
        self._check(L.icet_voxel_map_query_posed_device(self._h, len(outs), _vp(poses.data_ptr()), C.byref(q), O, _vp(d_rows_ptr), _vp(d_total_ptr), _vp(d_status_ptr)))

    def query(self, poses, min_range=0.0, max_range=0.0, min_points=1, world=False, cap_rows=None, static=False):
        """The host form: a count-only call, buffers of each query's total (or ``cap_rows``), the real call.  One dict per pose: xyz (n, 3) float32, count (n,)
        int64, key (n,) uint64, total, status."""
        import torch
        dev = torch.device("cuda", self._ctx.device)
        nq = int(poses.shape[0]) if hasattr(poses, "data_ptr") else np.asarray(poses, np.float32).reshape(-1, 16).shape[0]
        words = torch.zeros((3, max(nq, 1)), dtype=torch.int32, device=dev)      # rows | total | status
        torch.cuda.synchronize(dev)
        kw = dict(min_range=min_range, max_range=max_range, min_points=min_points, world=world, static=static)
        self.query_device(poses, [(None, 0, 0)] * nq, words[0].data_ptr(), d_total_ptr=words[1].data_ptr(), **kw)
        self._ctx.sync()
        caps = [int(t) if cap_rows is None else int(cap_rows) for t in words[1, :nq].cpu().numpy()]
        bufs = [(torch.zeros((3, max(c, 1)), dtype=torch.float32, device=dev), torch.zeros(max(c, 1), dtype=torch.int64, device=dev),
                 torch.zeros(max(c, 1), dtype=torch.int64, device=dev)) for c in caps]
        torch.cuda.synchronize(dev)
        outs = [(x.data_ptr() if c else None, max(c, 1), c, n.data_ptr(), k.data_ptr()) for c, (x, n, k) in zip(caps, bufs)]
        self.query_device(poses, outs, words[0].data_ptr(), d_total_ptr=words[1].data_ptr(), d_status_ptr=words[2].data_ptr(), **kw)
        self._ctx.sync()
        w = words.cpu().numpy()
        res = []
        for j, (x, n, k) in enumerate(bufs):
            r = int(w[0, j])
            res.append(dict(xyz=np.ascontiguousarray(x[:, :r].cpu().numpy().T), count=n[:r].cpu().numpy(), key=k[:r].cpu().numpy().view(np.uint64),
                            total=int(w[1, j]), status=int(w[2, j])))
        return res


class Deskewer:
    """``icet_deskewer`` (include/icet_hip.h): the rows of many scans, each with the motion of its own sweep as a twist, carried into the
    sensor frame at one instant of that sweep, in one launch on ``ctx``'s device.  The deskewer borrows ``ctx`` (closed before it)."""

    def __init__(self, ctx):
        self._ctx = ctx
        h = C.c_void_p()
        st = load_library().icet_deskewer_create(ctx._h, C.byref(h))
        if st != ICET_OK:
            raise IcetError(st, "icet_deskewer_create: " + load_library().icet_last_error(ctx._h).decode())
        self._h = h
        import weakref
        if not hasattr(ctx, "_nodes"):
            ctx._nodes = []
        ctx._nodes.append(weakref.ref(self))

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self._ctx, "_h", None):               # (a context finalised first took the device with it: see KeyframeStore.close)
                load_library().icet_deskewer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != ICET_OK:
            raise IcetError(st, load_library().icet_deskewer_last_error(self._h).decode())

    def deskew_device(self, scans, twists=None, d_counts_ptr=None):
        """One launch over ``scans`` (DeskewScan records of device memory: deskew_scan(); a list, or a ctypes array of them).  twists: None (the records' own), or a float64 CUDA tensor of
        n x 6 that replaces them.  d_counts_ptr: n DeskewCounts records in HBM, zeroed and filled in stream order.  Asynchronous on the context's stream."""
        A = scans if isinstance(scans, C.Array) else (DeskewScan * max(len(scans), 1))(*scans)      # (a caller that repeats a call keeps the array)
        tw = None
        if twists is not None:
            import torch
            if not (twists.is_cuda and twists.dtype == torch.float64 and twists.is_contiguous()) or twists.numel() != 6 * len(scans):
                raise IcetError(ICET_ERR_BAD_ARG, "device twists must be a contiguous float64 CUDA tensor of six values per scan")
            torch.cuda.current_stream(twists.device).synchronize()          # the context's stream is its own: the tensor must be complete
            tw = _vp(twists.data_ptr())
        self._check(load_library().icet_deskew_device(self._h, len(scans), A, tw, _vp(d_counts_ptr)))

    def deskew(self, scans, times, twists, ref=1.0, t0=0.0, span=1.0):
        """Host arrays: scans N_k x 3, times N_k (sweep time of every row; s = (time - t0) / span), twists n x 6.  Staged, synchronous.  Returns
        (the deskewed N_k x 3 float32 arrays, the counts as dicts)."""
        src = [_colmajor(s) for s in scans]
        tms = [np.ascontiguousarray(np.asarray(t, np.float32).reshape(-1)) for t in times]
        tw = np.asarray(twists, np.float64).reshape(-1, 6)
        if not (len(src) == len(tms) == tw.shape[0]) or any(a.shape[1] != t.shape[0] for a, t in zip(src, tms)):
            raise IcetError(ICET_ERR_BAD_ARG, "one time per row and one twist per scan")
        dst = [np.zeros_like(a) for a in src]
        recs = [deskew_scan(a.ctypes.data if a.size else 0, a.shape[1], a.shape[1], d.ctypes.data if d.size else 0, a.shape[1], t.ctypes.data if t.size else 0,
                            DESKEW_TIME_ARRAY, 0, t0, span, ref, x) for a, d, t, x in zip(src, dst, tms, tw)]
        A = (DeskewScan * max(len(recs), 1))(*recs)
        cnt = (DeskewCounts * max(len(recs), 1))()
        self._check(load_library().icet_deskew(self._h, len(recs), A, C.byref(cnt)))
        return [np.ascontiguousarray(d.T) for d in dst], [cnt[k].as_dict() for k in range(len(recs))]

    def twists_from_poses_device(self, d_poses_ptr, n, d_twists_ptr, scale=1.0):
        """d_twists[k] = scale log(T_k^-1 T_(k+1)), k < n, from n + 1 consecutive float32 4 x 4 poses in HBM (what optimize_pose_graph_device leaves there)
        into n x 6 float64 in HBM.  Asynchronous on the context's stream."""
        self._check(load_library().icet_deskew_twists_from_poses_device(self._h, int(n), _vp(d_poses_ptr), float(scale), _vp(d_twists_ptr)))


class MultiContext:
    """One context per GPU of this node (``icet_multi``): pair k of a batch runs on ``devices[k % len(devices)]``, results gathered."""

    def __init__(self, devices):
        L = load_library()
        ids = (C.c_int32 * max(len(devices), 1))(*[int(d) for d in devices])
        h = C.c_void_p()
        st = L.icet_multi_create(C.byref(h), ids, len(devices))
        if st != ICET_OK:
            raise IcetError(st, "icet_multi_create(%s)" % (list(devices),))
        self._h = h
        self.devices = list(devices)

    def close(self):
        if getattr(self, "_h", None):
            load_library().icet_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != ICET_OK:
            raise IcetError(st, load_library().icet_multi_last_error(self._h).decode())

    def solve_batch(self, scans1, scans2, runlen, X0=None, num_bins_phi=24, num_bins_theta=75, n=25, thresh=0.1, buff=0.1):
        k = len(scans1)
        p = Params(int(runlen), int(num_bins_phi), int(num_bins_theta), int(n), float(thresh), float(buff), 0)
        s1 = [_colmajor(s) for s in scans1]; s2 = [_colmajor(s) for s in scans2]
        a1 = (C.c_void_p * max(k, 1))(*[s.ctypes.data for s in s1]); a2 = (C.c_void_p * max(k, 1))(*[s.ctypes.data for s in s2])
        n1 = np.array([s.shape[1] for s in s1], np.int64); n2 = np.array([s.shape[1] for s in s2], np.int64)
        x0 = None if X0 is None else np.ascontiguousarray(np.asarray(X0, np.float32).reshape(k, 6))
        X = np.zeros((k, 6), np.float32); ps = np.zeros((k, 6), np.float32); cov = np.zeros((k, 36), np.float32)
        self._check(load_library().icet_multi_solve_batch(self._h, C.byref(p), k, a1, n1.ctypes.data, a2, n2.ctypes.data,
                                                          x0.ctypes.data if x0 is not None else None, X.ctypes.data, ps.ctypes.data, cov.ctypes.data))
        return dict(X=X, pred_stds=ps, cov=cov.reshape(k, 6, 6))

    def set_option(self, name, value):
        """"gather" (0 peer copies, 1 RCCL all-gather) or any per-context option, applied to every device (icet_multi_set_option)."""
        self._check(load_library().icet_multi_set_option(self._h, name.encode(), float(value)))

    def context_handle(self, i):
        return load_library().icet_multi_context(self._h, int(i))

    def context(self, i):
        """The context of devices[i] as a borrowed :class:`Context` (set_option / last_timing / reserve)."""
        return Context.borrow(self.context_handle(i), self.devices[i])

    def reserve(self, params, n_pairs, total_n1, total_n2):
        """Pre-size every device's workspace for its share of a batch (pairs round-robin: ceil(n_pairs / devices) each)."""
        L = load_library(); D = len(self.devices)
        for i in range(D):
            st = L.icet_reserve(C.c_void_p(self.context_handle(i)), C.byref(params), (n_pairs + D - 1) // D, (total_n1 + D - 1) // D + 1, (total_n2 + D - 1) // D + 1)
            if st != ICET_OK:
                raise IcetError(st, "icet_reserve on device entry %d" % i)

    def solve_batch_device(self, scan1_descs, scan2_descs, params, d_out_ptr, d_x0_ptr=None, producer_stream=None, asynchronous=False):
        """scan*_descs[k] = (device_ptr, n, ld) on devices[k % len(devices)]; d_out / d_x0 on devices[0].
        producer_stream: raw hipStream_t of devices[0] whose queued work (the writes of d_x0 / the scans) the solve must wait for.
        asynchronous=True returns as soon as the shares are handed to the device threads; call :meth:`sync` before reading d_out."""
        k = len(scan1_descs)
        A = _dev_scans(scan1_descs)
        B = _dev_scans(scan2_descs)
        fn = load_library().icet_multi_solve_batch_device_async if asynchronous else load_library().icet_multi_solve_batch_device_after
        self._check(fn(self._h, C.byref(params), k, A, B, C.c_void_p(d_x0_ptr) if d_x0_ptr else None, C.c_void_p(d_out_ptr),
                       C.c_void_p(producer_stream) if producer_stream else None))

    def sync(self):
        """icet_multi_sync: everything queued by asynchronous calls has completed on every device; raises the first failure."""
        self._check(load_library().icet_multi_sync(self._h))


_default_ctx = {}


def default_context(device=0):
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


def euler_R(phi, theta, psi):
    """utils::R (src/utils.cpp:144-152): body-frame xyz Euler rotation; used only to rebuild the ``points2`` member."""
    c, s = np.cos, np.sin
    return np.array([
        [c(theta) * c(psi), s(psi) * c(phi) + s(phi) * s(theta) * c(psi), s(phi) * s(psi) - s(theta) * c(phi) * c(psi)],
        [-s(psi) * c(theta), c(phi) * c(psi) - s(phi) * s(theta) * s(psi), s(phi) * c(psi) + s(theta) * s(psi) * c(phi)],
        [s(theta), -s(phi) * c(theta), c(phi) * c(theta)]], dtype=np.float32)


class ICET:
    """Drop-in mirror of the reference's ``ICET`` object (include/icet.h:36-116).

    ``ICET(scan1, scan2, runlen, X0, num_bins_phi, num_bins_theta, n=25, thresh=0.1, buff=0.1)`` -- the
    constructor runs the whole registration on the GPU; read ``X`` (x, y, z, roll, pitch, yaw) and
    ``pred_stds`` afterwards, exactly as odometry_node / map_maker_node do.  Also filled:
    ``clusterBounds`` (V x 6), ``points1``, ``points2`` (scan 2 under the transform of the LAST
    iteration, i.e. X before the final update -- src/icet.cpp:375-378 precede :433), ``HTWH_i``,
    ``HTWdz_i``, ``ellipsoid1Means`` / ``ellipsoid1Covariances`` / ``ellipsoid1Alphas``, and ``cov``
    (the full 6x6 the reference keeps only as a local).
    """

    def __init__(self, scan1, scan2, runlen, X0, num_bins_phi, num_bins_theta, n=25, thresh=0.1, buff=0.1, *, device=0, side_tables=True):
        """side_tables: False = X / pred_stds only; True = every member a caller in the reference reads; "full" = also the per-point members
        points1Spherical, pointIndices1, points2Spherical, pointIndices2 (include/icet.h:79,82,95-96: several MB more per solve)."""
        self.rl, self.numBinsPhi, self.numBinsTheta, self.n, self.thresh, self.buff = runlen, num_bins_phi, num_bins_theta, n, thresh, buff
        ctx = default_context(device)
        res = ctx.solve(scan1, scan2, runlen, X0, num_bins_phi, num_bins_theta, n, thresh, buff, aux=side_tables)
        self.X = res["X"]
        self.pred_stds = res["pred_stds"]
        self.cov = res["cov"]
        self.points1 = np.asarray(scan1, np.float32)
        if side_tables:
            a = res["aux"]
            self.clusterBounds = a["cluster_bounds"]
            self.testPoints = a["test_points"].reshape(-1, 3)           # (V * 6) x 3, src/icet.cpp:41,213-231 (zeros where the reference leaves garbage)
            fit = a["has_fit"] == 1
            self.ellipsoid1Means = list(a["mu1"][fit])
            self.ellipsoid1Covariances = list(a["sigma1"][fit])
            self.ellipsoid1Alphas = [0.3] * int(fit.sum())
            self.ellipsoid2Means, self.ellipsoid2Covariances, self.ellipsoid2Alphas = [], [], []   # always empty in the reference
            self.side = a
            if runlen > 0:
                self.HTWH_i = a["htwh"][runlen - 1]
                self.HTWdz_i = a["htwdz"][runlen - 1].reshape(6, 1)
                xprev = np.asarray(X0, np.float32).reshape(6) if runlen == 1 else a["x_hist"][runlen - 2]
                self.dx = a["x_hist"][runlen - 1] - xprev
                self.points2 = a["points2"]                  # (p + t) * R of the last iteration (src/icet.cpp:375-378)
                if side_tables == "full":
                    T, P = num_bins_theta, num_bins_phi
                    self.points1Spherical = a["points1_spherical"]; self.points2Spherical = a["points2_spherical"]
                    bs, idx = a["bin_start1"], a["point_index1"]
                    # [theta][phi] -> ascending indices, as std::vector<std::vector<std::vector<int>>> (include/icet.h:95-96)
                    self.pointIndices1 = [[idx[bs[T * ph + th]:bs[T * ph + th + 1]] for ph in range(P)] for th in range(T)]
                    order = np.argsort(a["voxel2"], kind="stable"); cnt = np.bincount(a["voxel2"], minlength=T * P); st = np.concatenate([[0], np.cumsum(cnt)])
                    self.pointIndices2 = [[order[st[T * ph + th]:st[T * ph + th + 1]] for ph in range(P)] for th in range(T)]


# ---------------------------------------------------------------------------------------------------------------------
# The callers around the constructor (include/icet_nodes.h): the per-frame body of the reference's odometry_node and
# map_maker_node (src/odometry.cpp:46-98, src/simpleMapMaker.cpp:86-172), state kept in HBM between frames.
ODOMETRY_NODE = dict(runlen=7, bins_phi=24, bins_theta=75, n=25, thresh=0.1, buff=0.1, min_range=2.0, seed_x0=1,
                     trans_thresh=0.0, rot_thresh=0.0, map_capacity=0, map_downsample=0)              # src/odometry.cpp:58,73-82
MAP_MAKER_NODE = dict(runlen=12, bins_phi=24, bins_theta=75, n=25, thresh=0.1, buff=0.1, min_range=0.2, seed_x0=0,
                      trans_thresh=0.3, rot_thresh=0.3, map_capacity=600000, map_downsample=2000)      # src/simpleMapMaker.cpp:62,98,113-124,147,241-242
NODE_NO_RANGE_FILTER, NODE_ALIGNED_CLOUD, NODE_SNAIL_TRAIL = 1, 2, 4
NODE_NO_PIPELINE, NODE_SERIAL_ENQUEUE, NODE_DOUBLE_W, NODE_TIME_PHASES = 8, 16, 32, 64      # include/icet_nodes.h
SCAN_REGISTRATION_NODE = dict(runlen=7, bins_phi=24, bins_theta=75, n=25, thresh=0.1, buff=0.1, min_range=0.0, seed_x0=0,
                              trans_thresh=0.0, rot_thresh=0.0, map_capacity=0, map_downsample=0, flags=7)  # src/scanMatcher.cpp:44,55-64,76,79-84


def node_params(**kw):
    d = dict(ODOMETRY_NODE); d.update(kw)
    return NodeParams(Params(d["runlen"], d["bins_phi"], d["bins_theta"], d["n"], d["thresh"], d["buff"], 0), d["min_range"], d["seed_x0"],
                      d["trans_thresh"], d["rot_thresh"], d["map_capacity"], d["map_downsample"], d.get("flags", 0))


def _result_dict(r):
    return dict(solved=bool(r.solved), diverged=bool(r.diverged), n_kept=int(r.n_kept), X=np.array(r.X[:], np.float32),
                pred_stds=np.array(r.pred_stds[:], np.float32), pose=np.array(r.pose[:], np.float32).reshape(4, 4),
                quat=np.array(r.quat[:], np.float32), map_rows=int(r.map_rows))


def debug_node_tail(X, pose):
    """icet_debug_node_tail (test hook, host only: no Context, no device): the scalars of a frame's tail as the node's frame_tail evaluates them, for the solution
    ``X`` (6) and the accumulated pose ``pose`` (4 x 4) before the frame -> dict(R (3, 3), Rinv (3, 3), pose (4, 4), quat (4: x, y, z, w)), float32."""
    x = np.ascontiguousarray(X, np.float32).reshape(6); p = np.ascontiguousarray(pose, np.float32).reshape(16)
    R, Ri, P, q = np.zeros(9, np.float32), np.zeros(9, np.float32), np.zeros(16, np.float32), np.zeros(4, np.float32)
    st = load_library().icet_debug_node_tail(x.ctypes.data, p.ctypes.data, R.ctypes.data, Ri.ctypes.data, P.ctypes.data, q.ctypes.data)
    if st != ICET_OK:
        raise IcetError(st, "icet_debug_node_tail")
    return dict(R=R.reshape(3, 3), Rinv=Ri.reshape(3, 3), pose=P.reshape(4, 4), quat=q)


class Node:
    """``icet_node``: feed lidar frames one by one; every frame after the first returns X, pred_stds and the chained pose."""

    def __init__(self, ctx=None, device=0, **kw):
        self._ctx = ctx if ctx is not None else Context(device)
        self._p = node_params(**kw)
        h = C.c_void_p()
        st = load_library().icet_node_create(self._ctx._h, C.byref(self._p), C.byref(h))
        if st != ICET_OK:
            raise IcetError(st, "icet_node_create")
        self._h = h
        import weakref
        if not hasattr(self._ctx, "_nodes"):
            self._ctx._nodes = []
        self._ctx._nodes.append(weakref.ref(self))

    def close(self):
        if getattr(self, "_h", None):
            load_library().icet_node_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def push(self, scan):
        """scan: N x 3 host array."""
        a = _colmajor(scan)
        r = NodeResult()
        st = load_library().icet_node_push(self._h, a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[1], C.byref(r))
        if st != ICET_OK:
            raise IcetError(st, "icet_node_push: " + (load_library().icet_node_last_error(self._h) or b"").decode())
        return _result_dict(r)

    def push_device(self, d_ptr, n, ld):
        """scan already in HBM on the context's device: column-major N x 3, leading dimension ld."""
        r = NodeResult()
        st = load_library().icet_node_push_device(self._h, C.c_void_p(int(d_ptr)), int(n), int(ld), C.byref(r))
        if st != ICET_OK:
            raise IcetError(st, "icet_node_push_device: " + (load_library().icet_node_last_error(self._h) or b"").decode())
        return _result_dict(r)

    def push_many_device(self, frames):
        """A burst of frames already in HBM, [(device_ptr, n, ld), ...]: icet_node_push_many_device -- pushed one after the other inside the library (one FFI call for all of them)."""
        k = len(frames)
        A = _dev_scans(frames)
        R = (NodeResult * max(k, 1))()
        st = load_library().icet_node_push_many_device(self._h, A, k, R)
        if st != ICET_OK:
            raise IcetError(st, "icet_node_push_many_device: " + (load_library().icet_node_last_error(self._h) or b"").decode())
        return [_result_dict(R[i]) for i in range(k)]

    def map(self):
        """``EigenQueue::getQueue()``: rows x 3, oldest first."""
        rows = C.c_int64()
        L = load_library()
        st = L.icet_node_map(self._h, None, 0, C.byref(rows))
        if st != ICET_OK:
            raise IcetError(st, "icet_node_map: " + (load_library().icet_node_last_error(self._h) or b"").decode())
        out = np.zeros((3, max(rows.value, 1)), np.float32)
        if rows.value:
            st = L.icet_node_map(self._h, out.ctypes.data_as(C.c_void_p), rows.value, C.byref(rows))
            if st != ICET_OK:
                raise IcetError(st, "icet_node_map: " + (load_library().icet_node_last_error(self._h) or b"").decode())
        return np.ascontiguousarray(out[:, :rows.value].T)

    def prev_scan(self):
        """The node's ``prev_pcl_matrix``: rows x 3."""
        rows = C.c_int64()
        L = load_library()
        st = L.icet_node_prev_scan(self._h, None, 0, C.byref(rows))
        if st != ICET_OK:
            raise IcetError(st, "icet_node_prev_scan: " + (load_library().icet_node_last_error(self._h) or b"").decode())
        out = np.zeros((3, max(rows.value, 1)), np.float32)
        if rows.value:
            st = L.icet_node_prev_scan(self._h, out.ctypes.data_as(C.c_void_p), rows.value, C.byref(rows))
            if st != ICET_OK:
                raise IcetError(st, "icet_node_prev_scan: " + (load_library().icet_node_last_error(self._h) or b"").decode())
        return np.ascontiguousarray(out[:, :rows.value].T)

    def _rows(self, fn, what):
        rows = C.c_int64()
        st = fn(self._h, None, 0, C.byref(rows))
        if st != ICET_OK:
            raise IcetError(st, what)
        out = np.zeros((3, max(rows.value, 1)), np.float32)
        if rows.value:
            st = fn(self._h, out.ctypes.data_as(C.c_void_p), rows.value, C.byref(rows))
            if st != ICET_OK:
                raise IcetError(st, what)
        return np.ascontiguousarray(out[:, :rows.value].T)

    def aligned(self):
        """``scan2_in_scan1_frame`` of the last frame (src/scanMatcher.cpp:76): rows x 3."""
        return self._rows(load_library().icet_node_aligned, "icet_node_aligned")

    def snail_trail(self):
        """``snailTrail`` (src/scanMatcher.cpp:79-84): rows x 3."""
        return self._rows(load_library().icet_node_snail_trail, "icet_node_snail_trail")

    def last_timing(self):
        t = (C.c_float * 3)()
        st = load_library().icet_node_last_timing(self._h, t)
        if st != ICET_OK:
            raise IcetError(st, "icet_node_last_timing: " + (load_library().icet_node_last_error(self._h) or b"").decode())
        return dict(filter_ms=t[0], solve_ms=t[1], map_ms=t[2])


class NodeGroup:
    """``icet_node_group``: ``n_streams`` independent nodes with one set of parameters (the presets above), advanced together.  Every call carries one frame for
    each of any subset of the streams and pays the frame's launch chain once; every stream gets the bits of its own :class:`Node` fed the same frames."""

    def __init__(self, ctx=None, n_streams=1, device=0, **kw):
        self._ctx = ctx if ctx is not None else Context(device)
        self._p = node_params(**kw)
        self.n_streams = int(n_streams)
        h = C.c_void_p()
        st = load_library().icet_node_group_create(self._ctx._h if self._ctx is not None else None, C.byref(self._p), self.n_streams, C.byref(h))
        if st != ICET_OK:
            raise IcetError(st, "icet_node_group_create")
        self._h = h
        import weakref
        if not hasattr(self._ctx, "_nodes"):
            self._ctx._nodes = []
        self._ctx._nodes.append(weakref.ref(self))

    def close(self):
        if getattr(self, "_h", None):
            load_library().icet_node_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, st, what):
        return IcetError(st, what + ": " + (load_library().icet_node_group_last_error(self._h) or b"").decode())

    def push_device(self, frames):
        """One frame for each of several streams, scans already in HBM on the context's device (and complete): [(stream, device_ptr, n, ld), ...] ->
        one result dict per frame, in the order given."""
        k = len(frames)
        ids = (C.c_int32 * max(k, 1))(*[int(f[0]) for f in frames])
        A = (DevScan * max(k, 1))(*[DevScan(int(p), int(n), int(ld)) for (_, p, n, ld) in frames])
        R = (NodeResult * max(k, 1))()
        st = load_library().icet_node_group_push_device(self._h, k, ids, A, R)
        if st != ICET_OK:
            raise self._err(st, "icet_node_group_push_device")
        return [_result_dict(R[i]) for i in range(k)]

    def _rows(self, fn, s, what):
        rows = C.c_int64()
        st = fn(self._h, int(s), None, 0, C.byref(rows))
        if st != ICET_OK:
            raise self._err(st, what)
        out = np.zeros((3, max(rows.value, 1)), np.float32)
        if rows.value:
            st = fn(self._h, int(s), out.ctypes.data_as(C.c_void_p), rows.value, C.byref(rows))
            if st != ICET_OK:
                raise self._err(st, what)
        return np.ascontiguousarray(out[:, :rows.value].T)

    def map(self, s):
        """Stream s's ``EigenQueue::getQueue()``: rows x 3, oldest first."""
        return self._rows(load_library().icet_node_group_map, s, "icet_node_group_map")

    def prev_scan(self, s):
        """Stream s's ``prev_pcl_matrix``: rows x 3."""
        return self._rows(load_library().icet_node_group_prev_scan, s, "icet_node_group_prev_scan")

    def aligned(self, s):
        """Stream s's ``scan2_in_scan1_frame`` of its last frame: rows x 3."""
        return self._rows(load_library().icet_node_group_aligned, s, "icet_node_group_aligned")

    def snail_trail(self, s):
        """Stream s's ``snailTrail``: rows x 3."""
        return self._rows(load_library().icet_node_group_snail_trail, s, "icet_node_group_snail_trail")


# ---------------------------------------------------------------------------------------------------------------------
# Scan files (include/icet_io.h): what utils::loadPointCloudCSV (src/utils.cpp:12-91) and the Python side's np.load / KITTI
# readers hand to the constructor.
FMT_AUTO, FMT_NPY, FMT_OUSTER_CSV, FMT_XYZ_TSV, FMT_KITTI_BIN = range(5)


def load_scan(path, fmt=FMT_AUTO):
    """-> N x 3 float32 array (row-major view of the library's column-major buffer)."""
    L = load_library()
    p = C.POINTER(C.c_float)(); n = C.c_int64()
    st = L.icet_load_scan(os.fsencode(path), int(fmt), C.byref(p), C.byref(n))
    if st != ICET_OK:
        raise IcetError(st, "icet_load_scan(%s)" % path)
    try:
        a = np.ctypeslib.as_array(p, shape=(3, max(n.value, 1)))[:, :n.value].T.copy()
    finally:
        L.icet_free_scan(p)
    return a


def save_scan_npy(path, scan):
    a = _colmajor(scan)
    st = load_library().icet_save_scan_npy(os.fsencode(path), a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[1])
    if st != ICET_OK:
        raise IcetError(st, "icet_save_scan_npy(%s)" % path)
