"""ctypes view of the C ABI (include/ergodic_amd.h) of the gfx950 engine.

This is plumbing for tests and bench.py: it loads ergodic_exploration_amd/lib/libergodic_amd.so
and fails loudly when the library is missing.  There is no CPU fallback: every compute
entry point runs HIP kernels on the device.
"""
import ctypes as C
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
# EEA_LIB_VARIANT selects an A/B build of the same sources (csrc/Makefile VARIANT=...)
LIB_PATH = os.path.join(_HERE, "lib", "libergodic_amd%s.so" % os.environ.get("EEA_LIB_VARIANT", ""))
HEADER_PATH = os.path.join(ROOT, "include", "ergodic_amd.h")

MODEL_OMNI, MODEL_SIMPLE_CART = 0, 1
PREC_F64, PREC_F32 = 0, 1
OK, ERR_INVALID_ARGUMENT, ERR_INVALID_TWIST, ERR_UNSUPPORTED, ERR_HIP, ERR_NO_TARGET, ERR_TIMEOUT = range(7)
# eea_set_option (process-wide dispatch options; the library reads no environment variable)
FIELD_DENSITY, FIELD_DEFICIT, FIELD_POTENTIAL = range(3)   # eea_field_kind (eea_records_field)
OPT_CONTROL_KERNEL, OPT_WORKGROUP_THREADS, OPT_COLLISION_IMPL, OPT_MAILBOX_POLL, OPT_REBUILD_IMPL, OPT_AGENT_LANES, OPT_RESIDENT_CONTROL, OPT_RESIDENT_IDLE_MS = range(8)


class EngineError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("eea status %d: %s" % (status, msg))
        self.status = status


class Config(C.Structure):
    _fields_ = [("model", C.c_int), ("precision", C.c_int), ("device", C.c_int),
                ("dt", C.c_double), ("horizon", C.c_double), ("resolution", C.c_double),
                ("expl_weight", C.c_double), ("num_basis", C.c_uint),
                ("Rinv", C.c_double * 9), ("umin", C.c_double * 3), ("umax", C.c_double * 3)]


class BatchIO(C.Structure):
    _fields_ = [("d_pose", C.c_void_p), ("d_ut", C.c_void_p), ("d_mem_cols", C.c_void_p),
                ("d_n_mem", C.c_void_p), ("mem_stride", C.c_uint), ("d_u0", C.c_void_p),
                ("d_traj", C.c_void_p), ("d_ck", C.c_void_p), ("d_edx", C.c_void_p),
                ("d_bdx", C.c_void_p), ("d_rhot", C.c_void_p), ("d_status", C.c_void_p),
                ("d_ck_shared", C.c_void_p), ("d_ck_rec", C.c_void_p), ("ck_shared_parts", C.c_uint),
                ("d_rec_ready", C.c_void_p), ("rec_seq", C.c_uint), ("d_ck_flag", C.c_void_p), ("ck_flag_seq", C.c_uint),
                ("d_skip", C.c_void_p), ("rec_per_wavefront", C.c_int)]


class ConsensusDesc(C.Structure):
    _fields_ = [("n_groups", C.c_uint), ("group_agents", C.POINTER(C.c_uint)), ("group_io", C.POINTER(BatchIO)),
                ("lag", C.c_uint), ("passes_per_launch", C.c_uint)]


class TickIO(C.Structure):
    _fields_ = [("d_follow_dwa", C.c_void_p), ("d_dwa_count", C.c_void_p), ("d_u", C.c_void_p), ("d_vb", C.c_void_p),
                ("d_grid", C.c_void_p), ("d_traj", C.c_void_p), ("d_valid", C.c_void_p), ("d_skip", C.c_void_p),
                ("d_source", C.c_void_p), ("val_dt", C.c_double), ("val_horizon", C.c_double), ("grid_epoch", C.c_ulonglong)]


class CollisionCfg(C.Structure):
    _fields_ = [("xmin", C.c_double), ("ymin", C.c_double), ("resolution", C.c_double),
                ("xsize", C.c_uint), ("ysize", C.c_uint), ("boundary_radius", C.c_double),
                ("search_radius", C.c_double), ("obstacle_threshold", C.c_double),
                ("occupied_threshold", C.c_double)]


class EvidenceCfg(C.Structure):
    """eea_evidence_cfg: w_occ / w_free evidence units for a hit / a miss, e_clip the clamp at publication, quantum log-odds per
    unit, thr_miss / thr_false the sensor's error probabilities times 2^32, (seed_lo, seed_hi) the key of the noise stream"""
    _fields_ = [("w_occ", C.c_int), ("w_free", C.c_int), ("e_clip", C.c_int), ("quantum", C.c_double),
                ("thr_miss", C.c_uint32), ("thr_false", C.c_uint32), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32)]


class Clearance(C.Structure):
    """eea_clearance: msg (COLLISION_*), sqrd_obs, dx, dy -- crash: 0, 0, 0; none: -1, 0, 0"""
    _fields_ = [("msg", C.c_int), ("sqrd_obs", C.c_int), ("dx", C.c_int), ("dy", C.c_int)]


COLLISION_CRASH, COLLISION_OBSTACLE, COLLISION_NONE = 0, 1, 2   # CollisionMsg (collision.hpp:55-60)
COLLISION_OFF_GRID = 3       # the distance queries only: the pose's cell is not on the grid
DISTANCE_MAX_SIDE = 8192     # EEA_DISTANCE_MAX_SIDE
GEODESIC_TILE_X, GEODESIC_TILE_Y = 32, 32           # EEA_GEODESIC_TILE_X / _Y: the tile of the geodesic field's rounds
GEODESIC_UNKNOWN_BLOCKS, GEODESIC_CONTINUE = 1, 2   # EEA_GEODESIC_*: flags of geodesic_field
GOTO_MAX_CELLS = 16384                              # EEA_GOTO_MAX_CELLS: the cells of a window of geodesic_goto_batch
GOTO_OK, GOTO_NO_ROBOT, GOTO_NO_GOAL, GOTO_WINDOW, GOTO_CUT_OFF = range(5)   # EEA_GOTO_*: a robot's status
FOOTPRINT_MAX_VERTICES = 16  # EEA_FOOTPRINT_MAX_VERTICES
FRONTIER_OF_GRID, FRONTIER_OF_MASK = 0, 1           # EEA_FRONTIER_OF_*: kind of frontier_regions


class FrontierRegion(C.Structure):
    """eea_frontier_region (56 bytes): sums of the members' rows / columns, the entry (cell, cost: one 8-byte word), root, size,
    the bounding box, the entry's owner, 0"""
    _fields_ = [("sum_i", C.c_uint64), ("sum_j", C.c_uint64), ("entry_cell", C.c_int32), ("entry_cost", C.c_int32),
                ("root", C.c_int32), ("size", C.c_uint32), ("i_min", C.c_int32), ("i_max", C.c_int32), ("j_min", C.c_int32),
                ("j_max", C.c_int32), ("entry_owner", C.c_int32), ("reserved", C.c_int32)]


class Footprint(C.Structure):
    """eea_footprint: n vertices in the body frame, counter-clockwise and strictly convex, the body origin strictly inside.
    Footprint.of(vertices) takes any number of (x, y) pairs up to the arrays' length (the library refuses n < 3)"""
    _fields_ = [("n", C.c_uint), ("x", C.c_double * FOOTPRINT_MAX_VERTICES), ("y", C.c_double * FOOTPRINT_MAX_VERTICES)]

    @classmethod
    def of(cls, vertices):
        fp = cls()
        fp.n = len(vertices)
        for k, (x, y) in enumerate(vertices[:FOOTPRINT_MAX_VERTICES]):
            fp.x[k], fp.y[k] = float(x), float(y)
        return fp


class DwaCfg(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("dt", "horizon", "acc_dt", "acc_lim_x", "acc_lim_y", "acc_lim_th",
                                          "max_vel_x", "min_vel_x", "max_vel_y", "min_vel_y",
                                          "max_rot_vel", "min_rot_vel")] + \
               [(n, C.c_uint) for n in ("vx_samples", "vy_samples", "vth_samples")]


def build(force=False):
    """hipcc --offload-arch=gfx950 build of the library (csrc/Makefile)."""
    args = ["make", "-s", "-j4", "-C", os.path.join(_HERE, "csrc")]
    if force:
        subprocess.check_call(args + ["clean"])
    subprocess.check_call(args)
    return LIB_PATH


def declared_symbols():
    """Entry points declared in include/ergodic_amd.h."""
    with open(HEADER_PATH) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(eea_[a-z0-9_]+)\s*\(", text)))


_lib = None


def lib():
    """Loads the shared library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libergodic_amd.so is missing: run __graft_entry__.build() "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        # One HIP runtime per process: the tests and bench.py hand torch-allocated device
        # memory and streams to the engine, so torch's bundled libamdhip64 must be the
        # instance this library binds to (loading the system one first gives two runtimes).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.eea_last_error.restype = C.c_char_p
        L.eea_steps.restype = C.c_uint
        L.eea_batch_agent_lanes.restype = C.c_uint
        L.eea_batch_agent_lanes.argtypes = [C.c_void_p, C.c_uint]
        L.eea_batch_record_count.restype = C.c_uint
        L.eea_batch_record_count.argtypes = [C.c_void_p, C.c_uint]
        L.eea_num_modes.restype = C.c_uint
        L.eea_real_size.restype = C.c_size_t
        L.eea_time_step.restype = C.c_double
        L.eea_abi_version.restype = C.c_uint
        L.eea_ck_record_len.restype = C.c_uint
        L.eea_ck_record_len.argtypes = [C.c_void_p]
        L.eea_ck_records_sum.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
        L.eea_ck_records_sum_bound.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
        L.eea_publish_record.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p]
        L.eea_stream_wait_flag.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p]
        L.eea_consensus_plan_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.eea_consensus_plan_launch.argtypes = [C.c_void_p, C.c_void_p]
        L.eea_consensus_plan_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_void_p)]
        L.eea_consensus_plan_destroy.argtypes = [C.c_void_p]
        L.eea_consensus_plan_destroy.restype = None
        L.eea_ck_records_sum_ws_bytes.argtypes = [C.c_void_p, C.c_uint, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.eea_ck_records_sum_ws.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("eea_steps", "eea_num_modes", "eea_real_size", "eea_time_step", "eea_destroy", "eea_resident_stop"):
            getattr(L, name).argtypes = [C.c_void_p]
        L.eea_destroy.restype = None
        L.eea_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
        L.eea_set_target_gaussians.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p]
        L.eea_set_target_grid.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_int,
                                          C.c_double, C.c_double, C.c_void_p]
        L.eea_spatial_coeff_rows.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_void_p,
                                             C.c_double, C.c_double, C.c_void_p, C.c_void_p]
        L.eea_set_target_occupancy.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_int,
                                               C.c_double, C.c_double, C.c_void_p]
        L.eea_spatial_coeff_occupancy_rows.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint,
                                                       C.c_void_p, C.c_double, C.c_double, C.c_void_p,
                                                       C.c_void_p]
        L.eea_set_phik.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double]
        L.eea_set_phik_from_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p]
        L.eea_config_domain.argtypes = [C.c_void_p] + [C.c_double] * 4 + [C.POINTER(C.c_int), C.c_void_p]
        L.eea_config_domain_async.argtypes = [C.c_void_p] + [C.c_double] * 4 + [C.POINTER(C.c_int), C.c_void_p]
        L.eea_get_phik.argtypes = [C.c_void_p, C.c_void_p]
        L.eea_get_lamdak.argtypes = [C.c_void_p, C.c_void_p]
        L.eea_target_grid_size.argtypes = [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
        L.eea_get_target_grid.argtypes = [C.c_void_p, C.c_void_p]
        L.eea_control_batch.argtypes = [C.c_void_p, C.c_uint, C.POINTER(BatchIO), C.c_void_p]
        L.eea_control_batch_steps.argtypes = [C.c_void_p, C.c_uint, C.POINTER(BatchIO), C.c_uint, C.c_uint, C.c_uint,
                                              C.c_void_p]
        L.eea_set_option.argtypes = [C.c_int, C.c_int]
        L.eea_get_option.argtypes = [C.c_int]
        if hasattr(L, "eea_debug_phase_timing"):  # A/B library only (EEA_LIB_VARIANT=_ab, tools/ab/)
            L.eea_debug_phase_timing.argtypes = [C.c_void_p, C.c_uint, C.POINTER(BatchIO), C.c_void_p, C.c_void_p]
        L.eea_comm_get_unique_id.argtypes = [C.c_void_p]
        L.eea_comm_set_library.argtypes = [C.c_char_p]
        L.eea_comm_set_library.restype = C.c_int
        L.eea_comm_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        L.eea_comm_destroy.argtypes = [C.c_void_p]
        L.eea_comm_destroy.restype = None
        L.eea_comm_rank.argtypes = [C.c_void_p]
        L.eea_comm_nranks.argtypes = [C.c_void_p]
        L.eea_ck_sum.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
        L.eea_comm_allgather_ck.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
        L.eea_comm_consensus_ck.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
        L.eea_comm_allreduce_sum_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_int]
        L.eea_comm_records_exchange_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_uint, C.c_int]
        L.eea_comm_wait.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.eea_comm_records_exchange_bound.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_uint,
                                                      C.c_void_p, C.c_void_p, C.c_int]
        L.eea_comm_allreduce_sum.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p]
        L.eea_comm_consensus_ck_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.eea_comm_allgather_ck_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.eea_comm_wait.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.eea_rollout_batch.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
        L.eea_control.argtypes = [C.c_void_p] + [C.c_double] * 4 + [C.c_void_p, C.c_void_p, C.c_uint,
                                                                     C.c_void_p]
        L.eea_opt_traj.argtypes = [C.c_void_p, C.c_void_p]
        L.eea_get_ut.argtypes = [C.c_void_p, C.c_void_p]
        L.eea_set_ut.argtypes = [C.c_void_p, C.c_void_p]
        L.eea_basis_traj_coeff.argtypes = [C.c_int, C.c_double, C.c_double, C.c_uint, C.c_void_p,
                                           C.c_uint, C.c_uint, C.c_void_p]
        L.eea_basis_spatial_coeff.argtypes = [C.c_int, C.c_double, C.c_double, C.c_uint, C.c_void_p,
                                              C.c_void_p, C.c_uint, C.c_void_p]
        L.eea_rk4_rollout.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        L.eea_target_fill.argtypes = [C.c_int, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p]
        L.eea_dwa_control_batch.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.POINTER(DwaCfg), C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint,
                                            C.c_double, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
        L.eea_collision_check_batch.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_void_p,
                                                C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p]
        L.eea_validate_control_batch.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                                 C.c_uint, C.c_void_p, C.c_void_p]
        if hasattr(L, "eea_clearance_batch"):   # additive to ABI 6: found by symbol (an older library variant has neither)
            L.eea_clearance_batch.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
            L.eea_clearance_field.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "eea_distance_field"):    # additive to ABI 6 as well
            L.eea_distance_field.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.eea_distance_query_batch.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.eea_distance_traj_min.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint,
                                                C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "eea_geodesic_field"):    # additive to ABI 6 as well
            L.eea_geodesic_ws_bytes.argtypes = [C.POINTER(CollisionCfg), C.POINTER(C.c_size_t)]
            L.eea_geodesic_field.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_void_p, C.c_void_p, C.c_int, C.c_uint, C.c_void_p,
                                             C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.eea_geodesic_path_batch.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_void_p, C.c_void_p, C.c_uint, C.c_uint,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]
            L.eea_set_target_reachable.argtypes = [C.c_void_p, C.POINTER(CollisionCfg), C.c_int, C.c_void_p, C.c_uint, C.c_void_p,
                                                   C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p]
        if hasattr(L, "eea_geodesic_partition"):    # additive to ABI 6 as well
            L.eea_partition_ws_bytes.argtypes = [C.POINTER(CollisionCfg), C.POINTER(C.c_size_t)]
            L.eea_geodesic_partition.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_void_p, C.c_void_p, C.c_int, C.c_uint,
                                                 C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
            L.eea_partition_goals.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_int, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_uint, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p]
            L.eea_partition_path_batch.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint,
                                                   C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "eea_frontier_regions"):    # additive to ABI 6 as well
            L.eea_frontier_ws_bytes.argtypes = [C.POINTER(CollisionCfg), C.POINTER(C.c_size_t)]
            L.eea_frontier_regions.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.eea_frontier_goals.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_double, C.c_double,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "eea_frontier_auction"):    # additive to ABI 6 as well
            L.eea_frontier_auction_ws_bytes.argtypes = [C.POINTER(CollisionCfg), C.c_uint, C.c_uint, C.POINTER(C.c_size_t)]
            L.eea_frontier_auction.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_void_p, C.c_void_p, C.c_int, C.c_uint, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint,
                                               C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "eea_geodesic_goto_batch"):    # additive to ABI 6 as well
            L.eea_geodesic_goto_batch.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_void_p, C.c_void_p, C.c_int, C.c_uint, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "eea_footprint_check_batch"):   # additive to ABI 6 as well
            L.eea_footprint_radii.argtypes = [C.POINTER(Footprint), C.POINTER(C.c_double), C.POINTER(C.c_double)]
            L.eea_footprint_check_batch.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.POINTER(Footprint), C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p]
            L.eea_footprint_traj_first.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.POINTER(Footprint), C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]
        if hasattr(L, "eea_footprint_dwa_control_batch"):   # additive to ABI 6 as well
            L.eea_footprint_validate_control_batch.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.POINTER(Footprint), C.c_void_p,
                                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_uint,
                                                               C.c_void_p, C.c_void_p]
            L.eea_footprint_dwa_control_batch.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.POINTER(DwaCfg), C.POINTER(Footprint),
                                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                          C.c_uint, C.c_double, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
            L.eea_tick_batch_footprint.argtypes = [C.c_void_p, C.c_uint, C.POINTER(BatchIO), C.POINTER(TickIO),
                                                   C.POINTER(CollisionCfg), C.POINTER(DwaCfg), C.POINTER(Footprint), C.c_void_p,
                                                   C.c_void_p]
        L.eea_replay_create.argtypes = [C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_uint64, C.c_uint, C.c_size_t, C.POINTER(C.c_void_p)]
        L.eea_replay_destroy.argtypes = [C.c_void_p]
        L.eea_replay_destroy.restype = None
        L.eea_replay_append.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.eea_replay_sample.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p]
        L.eea_replay_append_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint,
                                               C.c_void_p]
        L.eea_replay_counts.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)]
        L.eea_replay_read.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]
        L.eea_replay_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.eea_replay_pool_sample.argtypes = [C.c_void_p, C.c_uint64, C.c_uint, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint,
                                             C.c_void_p]
        L.eea_replay_history_records.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.eea_records_metric.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.eea_records_field.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint,
                                        C.c_void_p, C.c_void_p]
        L.eea_sense_ray_count.restype = C.c_uint
        L.eea_sense_ray_count.argtypes = [C.c_uint]
        L.eea_sense_reveal_batch.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p]
        L.eea_grid_census.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_void_p, C.c_void_p, C.c_void_p]
        L.eea_evidence_table.argtypes = [C.POINTER(EvidenceCfg), C.c_void_p]
        L.eea_sense_observe_batch.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.POINTER(EvidenceCfg), C.c_uint, C.c_uint, C.c_uint,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p]
        L.eea_evidence_publish.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.POINTER(EvidenceCfg), C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
        L.eea_sense_gain_field.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
        L.eea_set_target_gain.argtypes = [C.c_void_p, C.POINTER(CollisionCfg), C.c_uint, C.c_uint, C.c_void_p, C.c_double,
                                          C.c_double, C.c_double, C.c_void_p, C.c_void_p]
        L.eea_sense_mi_table.argtypes = [C.POINTER(CollisionCfg), C.c_double, C.c_void_p, C.c_void_p]
        L.eea_sense_mi_field.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_uint, C.c_uint, C.c_double, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
        L.eea_set_target_mi.argtypes = [C.c_void_p, C.POINTER(CollisionCfg), C.c_uint, C.c_uint, C.c_double, C.c_void_p, C.c_double,
                                        C.c_double, C.c_double, C.c_void_p, C.c_void_p]
        if hasattr(L, "eea_body_layer_create"):   # additive to ABI 6 as well
            L.eea_body_layer_create.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.POINTER(Footprint), C.c_uint, C.c_uint,
                                                C.POINTER(C.c_void_p)]
            L.eea_body_layer_destroy.argtypes = [C.c_void_p]
            L.eea_body_layer_destroy.restype = None
            L.eea_body_layer_update.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.eea_body_layer_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.eea_body_layer_box.argtypes = [C.c_void_p]
            L.eea_body_collision_check_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint,
                                                         C.c_void_p, C.c_void_p]
            L.eea_body_validate_control_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                          C.c_double, C.c_double, C.c_uint, C.c_void_p, C.c_void_p]
            L.eea_body_dwa_control_batch.argtypes = [C.c_void_p, C.POINTER(DwaCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_uint, C.c_double, C.c_void_p, C.c_uint,
                                                     C.c_void_p, C.c_void_p, C.c_void_p]
            L.eea_tick_batch_bodies.argtypes = [C.c_void_p, C.c_uint, C.POINTER(BatchIO), C.POINTER(TickIO),
                                                C.POINTER(CollisionCfg), C.POINTER(DwaCfg), C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "eea_fleet_layer_create"):   # additive to ABI 6: found by symbol (an older library has none of them)
            L.eea_fleet_layer_create.argtypes = [C.c_int, C.POINTER(CollisionCfg), C.c_int, C.c_uint, C.POINTER(C.c_void_p)]
            L.eea_fleet_layer_destroy.argtypes = [C.c_void_p]
            L.eea_fleet_layer_destroy.restype = None
            L.eea_fleet_layer_update.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.eea_fleet_layer_reach.argtypes = [C.c_void_p]
            L.eea_fleet_layer_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            L.eea_fleet_collision_check_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p]
            L.eea_tick_batch_fleet.argtypes = [C.c_void_p, C.c_uint, C.POINTER(BatchIO), C.POINTER(TickIO), C.POINTER(CollisionCfg),
                                               C.POINTER(DwaCfg), C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def check(status):
    if status != OK:
        raise EngineError(status, lib().eea_last_error().decode())


def make_config(model, dt, horizon, resolution, expl_weight, num_basis, Rinv, umin, umax,
                precision=PREC_F64, device=0):
    cfg = Config()
    cfg.model, cfg.precision, cfg.device = model, precision, device
    cfg.dt, cfg.horizon, cfg.resolution, cfg.expl_weight = dt, horizon, resolution, expl_weight
    cfg.num_basis = num_basis
    for c in range(3):
        for r in range(3):
            cfg.Rinv[r + 3 * c] = float(Rinv[r][c])
    for i in range(3):
        cfg.umin[i] = float(umin[i])
        cfg.umax[i] = float(umax[i])
    return cfg


def _ptr(t):
    """Raw device/host pointer of a torch tensor, numpy array or None."""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        return C.c_void_p(t.data_ptr())
    return C.c_void_p(t.ctypes.data)


class Engine:
    """One `ErgodicControl` engine (handle of the C ABI)."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.h = C.c_void_p()
        check(lib().eea_create(C.byref(cfg), C.byref(self.h)))
        self.T = int(lib().eea_steps(self.h))
        self.K2 = int(lib().eea_num_modes(self.h))
        self.real_size = int(lib().eea_real_size(self.h))

    def agent_lanes(self, B):
        """eea_batch_agent_lanes: lanes of a wavefront per agent for a plain batch of B agents (64, 8 / 16 / 32, or 0)"""
        return int(lib().eea_batch_agent_lanes(self.h, B))

    def record_count(self, B):
        """eea_batch_record_count: records a launch of B agents writes with rec_per_wavefront set (its wavefronts where agents
        share one, B otherwise)"""
        return int(lib().eea_batch_record_count(self.h, B))

    def close(self):
        if self.h:
            lib().eea_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_target_gaussians(self, mu, sigma):
        import numpy as np
        mu = np.ascontiguousarray(mu, dtype=np.float64).reshape(-1)
        sigma = np.ascontiguousarray(sigma, dtype=np.float64).reshape(-1)
        check(lib().eea_set_target_gaussians(self.h, mu.size // 2, _ptr(mu), _ptr(sigma)))

    def set_target_grid(self, nx, ny, phi_vals, lx, ly, stream=None):
        on_device = 1 if (hasattr(phi_vals, "is_cuda") and phi_vals.is_cuda) else 0
        check(lib().eea_set_target_grid(self.h, nx, ny, _ptr(phi_vals), on_device, lx, ly,
                                        C.c_void_p(stream or 0)))

    def spatial_coeff_rows(self, nx, ny_total, row0, nrows, phi_rows, lx, ly, out_partial, stream=None):
        """partial phi_k of the grid rows [row0, row0+nrows) held in the device tensor phi_rows"""
        check(lib().eea_spatial_coeff_rows(self.h, nx, ny_total, row0, nrows, _ptr(phi_rows), lx, ly,
                                           _ptr(out_partial), C.c_void_p(stream or 0)))

    def set_target_occupancy(self, nx, ny, occ, lx, ly, stream=None):
        """int8 occupancy cells (OccupancyGrid.data layout) -> entropy target -> phi_k, fused on the device"""
        on_device = 1 if (hasattr(occ, "is_cuda") and occ.is_cuda) else 0
        check(lib().eea_set_target_occupancy(self.h, nx, ny, _ptr(occ), on_device, lx, ly,
                                             C.c_void_p(stream or 0)))

    def set_target_gain(self, cfg, range_cells, stride, known, lx, ly, floor=0.0, gain=None, stream=None):
        """eea_set_target_gain: the information-gain field of the int8 device grid `known` (eea_sense_gain_field) + floor on
        the candidates -> phi_k, all on `stream` without a host wait; gain (optional, device uint32 [ysize][xsize]) receives
        the integer field"""
        check(lib().eea_set_target_gain(self.h, C.byref(cfg), int(range_cells), int(stride), _ptr(known), float(floor), lx, ly,
                                        _ptr(gain), C.c_void_p(stream or 0)))

    def set_target_mi(self, cfg, range_cells, stride, known, lx, ly, p_unknown=0.5, floor=0.0, mi=None, stream=None):
        """eea_set_target_mi: the mutual-information field of the int8 device grid `known` (eea_sense_mi_field) + floor on the
        candidates -> phi_k, all on `stream` without a host wait; mi (optional, device double [ysize][xsize]) receives the
        field"""
        check(lib().eea_set_target_mi(self.h, C.byref(cfg), int(range_cells), int(stride), float(p_unknown), _ptr(known),
                                      float(floor), lx, ly, _ptr(mi), C.c_void_p(stream or 0)))

    def set_target_reachable(self, cfg, kind, field, stride, known, geo, lx, ly, floor=0.0, stream=None):
        """eea_set_target_reachable: field (kind 0: the uint32 field of sense_gain_field, 1: the double field of sense_mi_field)
        + floor on the candidates of the int8 device grid `known` that do not block and have geo >= 0 (geodesic_field) -> phi_k,
        all on `stream` without a host wait"""
        check(lib().eea_set_target_reachable(self.h, C.byref(cfg), int(kind), _ptr(field), int(stride), _ptr(known), _ptr(geo),
                                             float(floor), lx, ly, C.c_void_p(stream or 0)))

    def spatial_coeff_occupancy_rows(self, nx, ny_total, row0, nrows, occ_rows, lx, ly, out_sums, stream=None):
        """un-normalised coefficient sums of the occupancy rows [row0, row0+nrows) (device int8 tensor)"""
        check(lib().eea_spatial_coeff_occupancy_rows(self.h, nx, ny_total, row0, nrows, _ptr(occ_rows), lx, ly,
                                                     _ptr(out_sums), C.c_void_p(stream or 0)))

    def set_phik(self, phik, lx, ly):
        on_device = 1 if (hasattr(phik, "is_cuda") and phik.is_cuda) else 0
        check(lib().eea_set_phik(self.h, _ptr(phik), on_device, lx, ly))

    def set_phik_from_sums(self, sums, lx, ly, stream=None):
        """phi_k = sums / sums[0] on the device, stream-ordered (grid-tiled occupancy target after the all-reduce)"""
        check(lib().eea_set_phik_from_sums(self.h, _ptr(sums), lx, ly, C.c_void_p(stream or 0)))

    def config_domain(self, bounds, stream=None):
        rebuilt = C.c_int(0)
        check(lib().eea_config_domain(self.h, *[float(b) for b in bounds], C.byref(rebuilt),
                                      C.c_void_p(stream or 0)))
        return bool(rebuilt.value)

    def config_domain_async(self, bounds, stream=None):
        """enqueue-only form: returns once the rebuild's launches are on the stream"""
        rebuilt = C.c_int(0)
        check(lib().eea_config_domain_async(self.h, *[float(b) for b in bounds], C.byref(rebuilt),
                                            C.c_void_p(stream or 0)))
        return bool(rebuilt.value)

    def phik(self):
        import numpy as np
        out = np.empty(self.K2)
        check(lib().eea_get_phik(self.h, _ptr(out)))
        return out

    def lamdak(self):
        import numpy as np
        out = np.empty(self.K2)
        check(lib().eea_get_lamdak(self.h, _ptr(out)))
        return out

    @property
    def target_grid_size(self):
        """(nx, ny) of the target grid of the last rebuild / eea_set_target_grid (eea_target_grid_size)"""
        nx, ny = C.c_uint(), C.c_uint()
        check(lib().eea_target_grid_size(self.h, C.byref(nx), C.byref(ny)))
        return nx.value, ny.value

    def target_grid(self):
        import numpy as np
        nx, ny = C.c_uint(), C.c_uint()
        check(lib().eea_target_grid_size(self.h, C.byref(nx), C.byref(ny)))
        out = np.empty(nx.value * ny.value)
        check(lib().eea_get_target_grid(self.h, _ptr(out)))
        return out, nx.value, ny.value

    def control_batch(self, B, pose, ut, u0, mem_cols=None, n_mem=None, mem_stride=0, traj=None,
                      ck=None, edx=None, bdx=None, rhot=None, status=None, stream=None, ck_shared=None,
                      ck_rec=None, ck_shared_parts=0, n_steps=None, pose_step_stride=0, u0_step_stride=0,
                      rec_ready=None, rec_seq=0, ck_flag=None, ck_flag_seq=0, skip=None,
                      rec_per_wavefront=False):
        """n_steps (ABI 4, eea_control_batch_steps): that many consecutive control() calls per agent in one launch;
        pose / u0 rows per step by the strides (in agents; 0 = the same row every step)."""
        io = BatchIO()
        io.d_ck_shared = _ptr(ck_shared)
        io.d_ck_rec, io.ck_shared_parts = _ptr(ck_rec), ck_shared_parts
        io.d_pose, io.d_ut, io.d_u0 = _ptr(pose), _ptr(ut), _ptr(u0)
        io.d_mem_cols, io.d_n_mem, io.mem_stride = _ptr(mem_cols), _ptr(n_mem), mem_stride
        io.d_traj, io.d_ck, io.d_edx, io.d_bdx = _ptr(traj), _ptr(ck), _ptr(edx), _ptr(bdx)
        io.d_rhot, io.d_status = _ptr(rhot), _ptr(status)
        io.d_rec_ready, io.rec_seq, io.d_ck_flag, io.ck_flag_seq = _ptr(rec_ready), rec_seq, _ptr(ck_flag), ck_flag_seq
        io.d_skip = _ptr(skip)
        io.rec_per_wavefront = 1 if rec_per_wavefront else 0
        if n_steps is None:
            check(lib().eea_control_batch(self.h, B, C.byref(io), C.c_void_p(stream or 0)))
        else:
            check(lib().eea_control_batch_steps(self.h, B, C.byref(io), n_steps, pose_step_stride, u0_step_stride,
                                                C.c_void_p(stream or 0)))

    def prepared_batch(self, B, pose, ut, u0, mem_cols=None, n_mem=None, mem_stride=0, ck=None, ck_shared=None,
                       stream=None, ck_rec=None, ck_shared_parts=0, n_steps=None, pose_step_stride=0, u0_step_stride=0,
                       rec_ready=None, ck_flag=None, status=None):
        """A callable that issues eea_control_batch with these (fixed) device buffers: one ctypes call per pass, the
        eea_batch_io is built once (a pass of 4096 agents takes ~30 us on the device; building the struct from
        tensors every pass costs about as much on the host)."""
        io = BatchIO()
        io.d_ck_shared = _ptr(ck_shared)
        io.d_pose, io.d_ut, io.d_u0 = _ptr(pose), _ptr(ut), _ptr(u0)
        io.d_mem_cols, io.d_n_mem, io.mem_stride = _ptr(mem_cols), _ptr(n_mem), mem_stride
        io.d_ck = _ptr(ck)
        io.d_ck_rec, io.ck_shared_parts = _ptr(ck_rec), ck_shared_parts
        io.d_rec_ready, io.d_ck_flag, io.d_status = _ptr(rec_ready), _ptr(ck_flag), _ptr(status)
        fn, h, ref, st = lib().eea_control_batch, self.h, C.byref(io), C.c_void_p(stream or 0)
        keep = (io, pose, ut, u0, mem_cols, n_mem, ck, ck_shared, ck_rec, rec_ready, ck_flag, status)
        if (rec_ready is not None or ck_flag is not None) and n_steps is not None:
            # (the engine's own answer for eea_control_batch_steps with the device-bound buffers, ergodic_amd.h)
            raise EngineError(ERR_UNSUPPORTED, "n_steps cannot be combined with rec_ready / ck_flag: a step must never wait "
                                               "for an exchange the host enqueues after the launch")
        if rec_ready is not None or ck_flag is not None:
            # device-bound exchange: the sequence numbers change from pass to pass -- call(rec_seq, ck_flag_seq)
            def call_bound(rec_seq=0, ck_flag_seq=0, _keep=keep):
                io.rec_seq, io.ck_flag_seq = rec_seq, ck_flag_seq
                rc = fn(h, B, ref, st)
                if rc != 0:
                    check(rc)
            return call_bound
        if n_steps is not None:   # ABI 4: n_steps receding-horizon steps per launch
            fns = lib().eea_control_batch_steps

            def call_steps(_keep=keep):
                rc = fns(h, B, ref, n_steps, pose_step_stride, u0_step_stride, st)
                if rc != 0:
                    check(rc)
            return call_steps

        def call(_keep=keep):
            rc = fn(h, B, ref, st)
            if rc != 0:
                check(rc)
        return call

    @property
    def ck_record_len(self):
        """reals per sum record (eea_batch_io::d_ck_rec): K^2 + 1 rounded up to even"""
        return int(lib().eea_ck_record_len(self.h))

    def ck_records_sum(self, B, recs, out, stream=None):
        """out[record_len] = sum of the B per-agent records (one launch, fixed order)"""
        check(lib().eea_ck_records_sum(self.h, B, _ptr(recs), _ptr(out), C.c_void_p(stream or 0)))

    def ck_records_sum_bound(self, B, recs, rec_ready, seq, out, flag=None, stream=None):
        """eea_ck_records_sum_bound: the sum polls the agents' ready marks (== seq) itself; flag (optional) = seq when done"""
        check(lib().eea_ck_records_sum_bound(self.h, B, _ptr(recs), _ptr(rec_ready), seq, _ptr(out), _ptr(flag),
                                             C.c_void_p(stream or 0)))

    def publish_record(self, src, pub, flag, seq, stream=None):
        check(lib().eea_publish_record(self.h, _ptr(src), _ptr(pub), _ptr(flag), seq, C.c_void_p(stream or 0)))

    def ck_sum(self, B, ck, sums, stream=None):
        """sums[:K2] = sum over the B agents of ck, sums[K2] = B (device tensors)"""
        check(lib().eea_ck_sum(self.h, B, _ptr(ck), _ptr(sums), C.c_void_p(stream or 0)))

    def debug_phase_timing(self, B, pose, ut, u0, stamps, ck=None, stream=None):
        """A/B library only (EEA_LIB_VARIANT=_ab): tools/phase_timing.py"""
        io = BatchIO()
        io.d_pose, io.d_ut, io.d_u0, io.d_ck = _ptr(pose), _ptr(ut), _ptr(u0), _ptr(ck)
        check(lib().eea_debug_phase_timing(self.h, B, C.byref(io), C.c_void_p(stream or 0), _ptr(stamps)))

    def _tick(self, symbol, extra, B, coll, dwa, stream, *io_args):
        """one tick entry: the two structs of io_args (_tick_io), `symbol` with `extra` between the window and the stream"""
        io, t = self._tick_io(*io_args)
        check(getattr(lib(), symbol)(self.h, B, C.byref(io), C.byref(t), C.byref(coll) if coll is not None else None, C.byref(dwa),
                                     *extra, C.c_void_p(stream or 0)))

    @staticmethod
    def _tick_io(pose, ut, follow, count, u, vb, grid, traj, valid, skip, val_dt, val_horizon, source, mem_cols, n_mem,
                 mem_stride, status, grid_epoch):
        io = BatchIO()
        io.d_pose, io.d_ut = _ptr(pose), _ptr(ut)
        io.d_mem_cols, io.d_n_mem, io.mem_stride, io.d_status = _ptr(mem_cols), _ptr(n_mem), mem_stride, _ptr(status)
        t = TickIO()
        t.d_follow_dwa, t.d_dwa_count, t.d_u, t.d_vb, t.d_grid = _ptr(follow), _ptr(count), _ptr(u), _ptr(vb), _ptr(grid)
        t.d_traj, t.d_valid, t.d_skip, t.d_source = _ptr(traj), _ptr(valid), _ptr(skip), _ptr(source)
        t.val_dt, t.val_horizon, t.grid_epoch = val_dt, val_horizon, grid_epoch
        return io, t

    def tick_batch(self, B, pose, ut, follow, count, u, vb, grid, traj, valid, skip, coll, dwa, val_dt, val_horizon,
                   source=None, mem_cols=None, n_mem=None, mem_stride=0, status=None, stream=None, grid_epoch=0):
        """eea_tick_batch: one iteration of Exploration::control's loop body (exploration.hpp:220-279) for B robots.
        coll / dwa: collision_cfg(...) / dwa_cfg(...)"""
        self._tick("eea_tick_batch", (), B, coll, dwa, stream, pose, ut, follow, count, u, vb, grid, traj, valid, skip, val_dt,
                   val_horizon, source, mem_cols, n_mem, mem_stride, status, grid_epoch)

    def tick_batch_fleet(self, layer, B, pose, ut, follow, count, u, vb, grid, traj, valid, skip, coll, dwa, val_dt, val_horizon,
                         source=None, mem_cols=None, n_mem=None, mem_stride=0, status=None, stream=None, grid_epoch=0):
        """eea_tick_batch_fleet: tick_batch with the FleetLayer `layer` in validate_control and the dynamic window -- the other
        robots' bodies are obstacles; robot r of the tick is robot r of the layer (updated on the same stream before)"""
        self._tick("eea_tick_batch_fleet", (layer.h if layer is not None else None,), B, coll, dwa, stream, pose, ut, follow, count,
                   u, vb, grid, traj, valid, skip, val_dt, val_horizon, source, mem_cols, n_mem, mem_stride, status, grid_epoch)

    def tick_batch_footprint(self, fp, B, pose, ut, follow, count, u, vb, grid, traj, valid, skip, coll, dwa, val_dt, val_horizon,
                             sq=None, source=None, mem_cols=None, n_mem=None, mem_stride=0, status=None, stream=None):
        """eea_tick_batch_footprint: tick_batch with the polygon base fp (a Footprint) in validate_control and the dynamic
        window; sq: the int32 plane of distance_field for the grid (rebuilt by the caller when the grid changes) or None"""
        self._tick("eea_tick_batch_footprint", (C.byref(fp) if fp is not None else None, _ptr(sq)), B, coll, dwa, stream, pose, ut,
                   follow, count, u, vb, grid, traj, valid, skip, val_dt, val_horizon, source, mem_cols, n_mem, mem_stride, status, 0)

    def tick_batch_bodies(self, layer, B, pose, ut, follow, count, u, vb, grid, traj, valid, skip, coll, dwa, val_dt, val_horizon,
                          sq=None, source=None, mem_cols=None, n_mem=None, mem_stride=0, status=None, stream=None):
        """eea_tick_batch_bodies: tick_batch_footprint with the BodyLayer `layer` in validate_control and the dynamic window --
        the other robots' polygon bodies are obstacles; robot r of the tick is robot r of the layer (updated on the same
        stream before).  The footprint is the layer's"""
        self._tick("eea_tick_batch_bodies", (layer.h if layer is not None else None, _ptr(sq)), B, coll, dwa, stream, pose, ut,
                   follow, count, u, vb, grid, traj, valid, skip, val_dt, val_horizon, source, mem_cols, n_mem, mem_stride, status, 0)

    def rollout_batch(self, B, pose, ut, traj, status=None, stream=None):
        check(lib().eea_rollout_batch(self.h, B, _ptr(pose), _ptr(ut), _ptr(traj), _ptr(status),
                                      C.c_void_p(stream or 0)))

    def control(self, bounds, x, mem_cols=None):
        """Single agent, host buffers: mirrors ErgodicControl::control(grid, x)."""
        import numpy as np
        x = np.ascontiguousarray(x, dtype=np.float64)
        u = np.empty(3)
        n_mem, mem = 0, None
        if mem_cols is not None and np.asarray(mem_cols).size:
            mem = np.ascontiguousarray(np.asarray(mem_cols, dtype=np.float64).T)  # (n_mem, 3)
            n_mem = mem.shape[0]
        check(lib().eea_control(self.h, *[float(b) for b in bounds], _ptr(x), _ptr(mem), n_mem,
                                _ptr(u)))
        return u

    def resident_stop(self):
        """eea_resident_stop: the resident single-robot workgroup (OPT_RESIDENT_CONTROL) leaves now; the next control() starts
        another one"""
        check(lib().eea_resident_stop(self.h))

    def opt_traj(self):
        import numpy as np
        out = np.empty((self.T, 3))
        check(lib().eea_opt_traj(self.h, _ptr(out)))
        return out.T.copy()

    def get_ut(self):
        import numpy as np
        out = np.empty((self.T, 3))
        check(lib().eea_get_ut(self.h, _ptr(out)))
        return out.T.copy()

    def set_ut(self, ut):
        import numpy as np
        a = np.ascontiguousarray(np.asarray(ut, dtype=np.float64).T)
        check(lib().eea_set_ut(self.h, _ptr(a)))


def basis_traj_coeff(lx, ly, K, xt, device=0):
    import numpy as np
    xt = np.asarray(xt, dtype=np.float64)
    rows, n = xt.shape
    a = np.ascontiguousarray(xt.T)
    out = np.empty(K * K)
    check(lib().eea_basis_traj_coeff(device, lx, ly, K, _ptr(a), rows, n, _ptr(out)))
    return out


def basis_spatial_coeff(lx, ly, K, phi_vals, grid, device=0):
    import numpy as np
    pv = np.ascontiguousarray(phi_vals, dtype=np.float64)
    g = np.ascontiguousarray(np.asarray(grid, dtype=np.float64).T)
    out = np.empty(K * K)
    check(lib().eea_basis_spatial_coeff(device, lx, ly, K, _ptr(pv), _ptr(g), pv.size, _ptr(out)))
    return out


def rk4_rollout(model, dt, horizon, x0, ut, device=0):
    """RungeKutta::solve for Omni / SimpleCart on the device. ut (3, T) -> xt (3, T)"""
    import numpy as np
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    a = np.ascontiguousarray(np.asarray(ut, dtype=np.float64).T)
    T = a.shape[0]
    out = np.empty((T, 3))
    check(lib().eea_rk4_rollout(device, model, dt, horizon, _ptr(x0), _ptr(a), _ptr(out)))
    return out.T.copy()


def target_fill(mu, sigma, trans, grid, device=0):
    import numpy as np
    mu = np.ascontiguousarray(mu, dtype=np.float64).reshape(-1)
    sigma = np.ascontiguousarray(sigma, dtype=np.float64).reshape(-1)
    trans = np.ascontiguousarray(trans, dtype=np.float64)
    g = np.ascontiguousarray(np.asarray(grid, dtype=np.float64).T)
    out = np.empty(g.shape[0])
    check(lib().eea_target_fill(device, mu.size // 2, _ptr(mu), _ptr(sigma), _ptr(trans), _ptr(g),
                                g.shape[0], _ptr(out)))
    return out


def make_collision_cfg(xmin, ymin, resolution, xsize, ysize, boundary_radius, search_radius,
                       obstacle_threshold, occupied_threshold):
    return CollisionCfg(xmin, ymin, resolution, xsize, ysize, boundary_radius, search_radius,
                        obstacle_threshold, occupied_threshold)


def collision_check_batch(cfg, grid, pose, hit, device=0, stream=None):
    check(lib().eea_collision_check_batch(device, C.byref(cfg), _ptr(grid), _ptr(pose),
                                          pose.shape[0], _ptr(hit), C.c_void_p(stream or 0)))


def validate_control_batch(cfg, grid, x0, u, dt, horizon, valid, device=0, stream=None):
    check(lib().eea_validate_control_batch(device, C.byref(cfg), _ptr(grid), _ptr(x0), _ptr(u), dt,
                                           horizon, x0.shape[0], _ptr(valid),
                                           C.c_void_p(stream or 0)))


def dwa_control_batch(ccfg, dcfg, grid, x0, vb, u_opt, found, vref=None, xt_ref=None, dt_ref=0.0, device=0,
                      stream=None):
    """DynamicWindow::control for P robots; xt_ref device tensor [P][n_ref][3] or None"""
    n_ref = xt_ref.shape[1] if xt_ref is not None else 0
    check(lib().eea_dwa_control_batch(device, C.byref(ccfg), C.byref(dcfg), _ptr(grid), _ptr(x0), _ptr(vb),
                                      _ptr(vref), _ptr(xt_ref), n_ref, dt_ref, x0.shape[0], _ptr(u_opt),
                                      _ptr(found), C.c_void_p(stream or 0)))


def clearance_batch(cfg, grid, pose, out, dmin=None, disp=None, device=0, stream=None):
    """eea_clearance_batch: Collision::minDistance + minDirection of the P poses pose [P][3] on the int8 device grid.  out: int32
    [P][4] (one Clearance per pose: msg, sqrd_obs, dx, dy), dmin: float64 [P], disp: float64 [P][2]; each may be None, not all
    three.  Device tensors; asynchronous"""
    check(lib().eea_clearance_batch(device, C.byref(cfg), _ptr(grid), _ptr(pose), int(pose.shape[0]), _ptr(out), _ptr(dmin),
                                    _ptr(disp), C.c_void_p(stream or 0)))


def clearance_field(cfg, grid, field=None, dmin=None, device=0, stream=None):
    """eea_clearance_field: the same for the centre of every cell; field: int32 [ysize][xsize][4], dmin: float64 [ysize][xsize];
    either may be None, not both.  Device tensors; asynchronous"""
    check(lib().eea_clearance_field(device, C.byref(cfg), _ptr(grid), _ptr(field), _ptr(dmin), C.c_void_p(stream or 0)))


def distance_field(cfg, grid, sq, nearest=None, device=0, stream=None):
    """eea_distance_field: the exact Euclidean distance transform of the occupied cells of the int8 device grid.  sq: int32
    [ysize][xsize] squared cell distances (-1 everywhere: no occupied cell), nearest: int32 [ysize][xsize] row-major index of
    the nearest occupied cell (the smallest among equals) or None.  Device tensors; asynchronous"""
    check(lib().eea_distance_field(device, C.byref(cfg), _ptr(grid), _ptr(sq), _ptr(nearest), C.c_void_p(stream or 0)))


def distance_query_batch(cfg, sq, nearest, pose, out=None, dmin=None, disp=None, device=0, stream=None):
    """eea_distance_query_batch: the P poses pose [P][3] through a built field.  out: int32 [P][4] (msg incl.
    COLLISION_OFF_GRID, sqrd_obs, dx, dy), dmin: float64 [P], disp: float64 [P][2]; each may be None, not all three; nearest may
    be None when out and disp are.  Device tensors; asynchronous"""
    check(lib().eea_distance_query_batch(device, C.byref(cfg), _ptr(sq), _ptr(nearest), _ptr(pose), int(pose.shape[0]), _ptr(out),
                                         _ptr(dmin), _ptr(disp), C.c_void_p(stream or 0)))


def distance_traj_min(cfg, sq, nearest, traj, out=None, step=None, dmin=None, device=0, stream=None):
    """eea_distance_traj_min: the worst step of each of the B trajectories traj [B][T][3] through a built field.  out: int32
    [B][4], step: int32 [B], dmin: float64 [B]; each may be None, not all three; nearest may be None when out is.  Device
    tensors; asynchronous"""
    check(lib().eea_distance_traj_min(device, C.byref(cfg), _ptr(sq), _ptr(nearest), _ptr(traj), int(traj.shape[0]),
                                      int(traj.shape[1]), _ptr(out), _ptr(step), _ptr(dmin), C.c_void_p(stream or 0)))


def geodesic_ws_bytes(cfg):
    """eea_geodesic_ws_bytes: the bytes of workspace geodesic_field needs for the grid of cfg; host only"""
    n = C.c_size_t()
    check(lib().eea_geodesic_ws_bytes(C.byref(cfg), C.byref(n)))
    return n.value


def geodesic_field(cfg, grid, geo, ws, state, pose=None, cells=None, sq=None, clear_sq=0, flags=0, max_rounds=0, device=0,
                   stream=None):
    """eea_geodesic_field: geo int32 [ysize][xsize] = the 5-7 chamfer cost of the cheapest move sequence through traversable
    cells of the int8 device grid from the cells of pose [P][3] and / or the row-major indices cells (int32), -1 where there is
    none.  sq: the int32 plane of distance_field for the same grid (cells within clear_sq of an occupied one are not
    traversable) or None; ws: geodesic_ws_bytes(cfg) bytes; state: uint32 [4] (final, rounds that changed something, accepted
    sources, 0).  max_rounds == 0 runs to the end and waits on the stream; max_rounds > 0 enqueues at most that many rounds
    and does not wait.  Device tensors"""
    check(lib().eea_geodesic_field(device, C.byref(cfg), _ptr(grid), _ptr(sq), int(clear_sq), int(flags), _ptr(pose),
                                   0 if pose is None else int(pose.shape[0]), _ptr(cells), 0 if cells is None else int(cells.shape[0]),
                                   int(max_rounds), _ptr(geo), _ptr(ws), _ptr(state), C.c_void_p(stream or 0)))


def geodesic_path_batch(cfg, geo, pose, path, length=None, device=0, stream=None):
    """eea_geodesic_path_batch: path float64 [P][n_steps][3] = the descent of geo from each pose of pose [P][3] as way-points
    (cell centres, the heading of the move), padded with the last one -- the layout xt_ref of dwa_control_batch reads; length:
    int32 [P] (moves written, -1: the pose is off the grid or unreachable) or None.  Device tensors; asynchronous"""
    check(lib().eea_geodesic_path_batch(device, C.byref(cfg), _ptr(geo), _ptr(pose), int(pose.shape[0]), int(path.shape[1]),
                                        _ptr(path), _ptr(length), C.c_void_p(stream or 0)))


def partition_ws_bytes(cfg):
    """eea_partition_ws_bytes: the bytes of workspace geodesic_partition needs for the grid of cfg; host only"""
    n = C.c_size_t()
    check(lib().eea_partition_ws_bytes(C.byref(cfg), C.byref(n)))
    return n.value


def geodesic_partition(cfg, grid, geo, owner, ws, state, pose=None, cells=None, sq=None, clear_sq=0, flags=0, max_rounds=0,
                       device=0, stream=None):
    """eea_geodesic_partition: geodesic_field's geo int32 [ysize][xsize] for the same arguments, and owner int32 [ysize][xsize]
    = the label of the source that reaches the cell most cheaply (pose q has label q, cell k label P + k; the smallest label
    among those at that cost), -1 where geo is -1.  ws: partition_ws_bytes(cfg) bytes, 8-byte aligned; state, max_rounds, flags
    as geodesic_field (GEODESIC_CONTINUE rebuilds from geo AND owner).  Device tensors"""
    check(lib().eea_geodesic_partition(device, C.byref(cfg), _ptr(grid), _ptr(sq), int(clear_sq), int(flags), _ptr(pose),
                                       0 if pose is None else int(pose.shape[0]), _ptr(cells),
                                       0 if cells is None else int(cells.shape[0]), int(max_rounds), _ptr(geo), _ptr(owner), _ptr(ws),
                                       _ptr(state), C.c_void_p(stream or 0)))


def partition_goals(cfg, kind, field, stride, known, geo, owner, goal_cell, goal_score, area, w_field=1.0, w_cost=0.0, device=0,
                    stream=None):
    """eea_partition_goals: per label r < len(goal_cell): area uint32 [n] = the cells owner r holds; goal_cell int32 [n] = the
    candidate of r (owner r, on the stride lattice, not blocking in the int8 grid `known`, field > 0) with the greatest
    w_field * field - w_cost * geo, the lowest index on a tie, -1 for none; goal_score float64 [n] = that score or 0.0.  kind 0:
    field is the uint32 field of sense_gain_field, 1: the double field of sense_mi_field.  Device tensors; asynchronous"""
    check(lib().eea_partition_goals(device, C.byref(cfg), int(kind), _ptr(field), int(stride), _ptr(known), _ptr(geo), _ptr(owner),
                                    int(goal_cell.shape[0]), float(w_field), float(w_cost), _ptr(goal_cell), _ptr(goal_score),
                                    _ptr(area), C.c_void_p(stream or 0)))


def partition_path_batch(cfg, geo, owner, pose, goal_cell, path, length=None, device=0, stream=None):
    """eea_partition_path_batch: path float64 [P][n_steps][3] = robot q's way from its own cell to goal_cell[q] inside its own
    region of owner (way-points as geodesic_path_batch's, headings of the forward moves), padded with the last one; length: int32
    [P] (moves written, -1: no such way) or None.  Device tensors; asynchronous"""
    check(lib().eea_partition_path_batch(device, C.byref(cfg), _ptr(geo), _ptr(owner), _ptr(pose), int(pose.shape[0]),
                                         _ptr(goal_cell), int(path.shape[1]), _ptr(path), _ptr(length), C.c_void_p(stream or 0)))


def frontier_ws_bytes(cfg):
    """eea_frontier_ws_bytes: the bytes of workspace frontier_regions needs for the grid of cfg; host only"""
    n = C.c_size_t()
    check(lib().eea_frontier_ws_bytes(C.byref(cfg), C.byref(n)))
    return n.value


def frontier_regions(cfg, kind, grid, root, region, ws, state, regions=None, max_regions=0, geo=None, owner=None, device=0,
                     stream=None):
    """eea_frontier_regions: the members of the int8 device grid (FRONTIER_OF_GRID: free cells with an unknown axis neighbour;
    FRONTIER_OF_MASK: non-zero cells; with geo also geo >= 0) in 8-connected regions.  root / region int32 [ysize][xsize] = the
    least index / the rank of the cell's region, -1 for a non-member; regions: max_regions records of sizeof(FrontierRegion)
    bytes (any dtype) or None with max_regions 0; state uint32 [4] (regions, records written, members, 0); ws:
    frontier_ws_bytes(cfg) bytes, 8-byte aligned.  Device tensors; asynchronous"""
    check(lib().eea_frontier_regions(device, C.byref(cfg), int(kind), _ptr(grid), _ptr(geo), _ptr(owner), int(max_regions), _ptr(root),
                                     _ptr(region), _ptr(regions), _ptr(ws), _ptr(state), C.c_void_p(stream or 0)))


def frontier_goals(regions, state, max_regions, goal_cell, goal_region, goal_score, min_size=1, w_size=1.0, w_cost=0.0, device=0,
                   stream=None):
    """eea_frontier_goals: per robot q < len(goal_cell) the record r < state[1] with entry_owner q, an entry and size >= min_size
    of the greatest w_size * size - w_cost * entry_cost, the lowest r on a tie: goal_cell int32 = its entry_cell or -1,
    goal_region int32 = r or -1, goal_score float64 = the score or 0.0.  Device tensors; asynchronous"""
    check(lib().eea_frontier_goals(device, _ptr(regions), _ptr(state), int(max_regions), int(goal_cell.shape[0]), int(min_size),
                                   float(w_size), float(w_cost), _ptr(goal_cell), _ptr(goal_region), _ptr(goal_score),
                                   C.c_void_p(stream or 0)))


def frontier_auction_ws_bytes(cfg, P, max_regions):
    """eea_frontier_auction_ws_bytes: the bytes of workspace frontier_auction needs for the grid of cfg, P robots and
    max_regions records; host only"""
    n = C.c_size_t()
    check(lib().eea_frontier_auction_ws_bytes(C.byref(cfg), int(P), int(max_regions), C.byref(n)))
    return n.value


def frontier_auction(cfg, grid, region, regions, fstate, max_regions, pose, goal_region, goal_cell, goal_cost, ws, state, path=None,
                     length=None, sq=None, clear_sq=0, flags=0, n_auction=1, min_size=1, cells_per_robot=0, max_rounds=0, device=0,
                     stream=None):
    """eea_frontier_auction: per robot of pose [P][3] a region of one frontier_regions call on the same int8 device grid (its
    rank plane region, its records regions or None with max_regions 0, its state fstate), by n_auction rounds of: the partition
    sourced at the open regions, a bid of every unassigned robot for its nearest one, and each region taking the nearest
    bidders it has room for (1, or ceil(size / cells_per_robot)).  goal_region / goal_cell / goal_cost int32 [P] (-1: none); path
    float64 [P][n_steps][3] (or None: n_steps 0) = the way to goal_cell as geodesic_path_batch's rows; length int32 [P] or None;
    ws: frontier_auction_ws_bytes(cfg, P, max_regions) bytes, 8-byte aligned; state uint32 [4] (every build final, tile rounds
    that changed something, robots assigned, rounds that were not idle).  max_rounds == 0 builds every field to the end and
    waits on the stream; max_rounds > 0 enqueues that many tile rounds per auction round and does not wait.  Device tensors"""
    check(lib().eea_frontier_auction(device, C.byref(cfg), _ptr(grid), _ptr(sq), int(clear_sq), int(flags), _ptr(region), _ptr(regions),
                                     _ptr(fstate), int(max_regions), _ptr(pose), 0 if pose is None else int(pose.shape[0]),
                                     int(n_auction), int(min_size), int(cells_per_robot), int(max_rounds),
                                     0 if path is None else int(path.shape[1]), _ptr(goal_region), _ptr(goal_cell), _ptr(goal_cost),
                                     _ptr(path), _ptr(length), _ptr(ws), _ptr(state), C.c_void_p(stream or 0)))


def geodesic_goto_batch(cfg, grid, pose, goal, cost, status, state, path=None, length=None, mask=None, sq=None, clear_sq=0, flags=0,
                        margin=0, device=0, stream=None):
    """eea_geodesic_goto_batch: per robot of pose [P][3] the shortest 5-7 chamfer path to its own cell goal[q] (int32 [P], row-major)
    inside the window of the two cells grown by margin and clipped to the int8 device grid (at most GOTO_MAX_CELLS cells).  cost
    int32 [P] = the path's cost or -1; status int32 [P] = GOTO_OK / _NO_ROBOT / _NO_GOAL / _WINDOW / _CUT_OFF; path float64
    [P][n_steps][3] (or None: n_steps 0) = geodesic_path_batch's rows; length int32 [P] or None; mask int32 [P] or None (0 leaves
    a robot out: nothing of it is read or written); state uint32 [4] = the robots OK, WINDOW, CUT_OFF, NO_ROBOT + NO_GOAL.  sq,
    clear_sq, flags (GEODESIC_UNKNOWN_BLOCKS only) as geodesic_field.  No workspace.  Device tensors; asynchronous"""
    if not hasattr(lib(), "eea_geodesic_goto_batch"):
        raise RuntimeError("libergodic_amd.so has no eea_geodesic_goto_batch: rebuild it (there is no fallback)")
    check(lib().eea_geodesic_goto_batch(device, C.byref(cfg), _ptr(grid), _ptr(sq), int(clear_sq), int(flags), _ptr(pose), _ptr(goal),
                                        _ptr(mask), 0 if pose is None else int(pose.shape[0]), int(margin),
                                        0 if path is None else int(path.shape[1]), _ptr(cost), _ptr(status), _ptr(path), _ptr(length),
                                        _ptr(state), C.c_void_p(stream or 0)))


def footprint_radii(fp):
    """eea_footprint_radii: (r_in, r_out) of the inscribed and the circumscribed circle about the body origin; validates the
    footprint on the host, needs no device"""
    r_in, r_out = C.c_double(), C.c_double()
    check(lib().eea_footprint_radii(C.byref(fp), C.byref(r_in), C.byref(r_out)))
    return r_in.value, r_out.value


def footprint_check_batch(cfg, fp, grid, pose, hit, sq=None, device=0, stream=None):
    """eea_footprint_check_batch: hit int32 [P] = 1 / 0 per pose of pose [P][3] for the polygon base fp on the int8 device grid;
    sq: the int32 plane of distance_field for the same grid (the filter) or None (every pose takes the exact test).  Device
    tensors; asynchronous"""
    check(lib().eea_footprint_check_batch(device, C.byref(cfg), C.byref(fp), _ptr(grid), _ptr(sq), _ptr(pose), int(pose.shape[0]),
                                          _ptr(hit), C.c_void_p(stream or 0)))


def footprint_traj_first(cfg, fp, grid, traj, step, sq=None, device=0, stream=None):
    """eea_footprint_traj_first: step int32 [B] = the first colliding step of each trajectory traj [B][T][3], -1: none; sq as in
    footprint_check_batch.  Device tensors; asynchronous"""
    check(lib().eea_footprint_traj_first(device, C.byref(cfg), C.byref(fp), _ptr(grid), _ptr(sq), _ptr(traj), int(traj.shape[0]),
                                         int(traj.shape[1]), _ptr(step), C.c_void_p(stream or 0)))


def footprint_validate_control_batch(cfg, fp, grid, x0, u, dt, horizon, valid, sq=None, device=0, stream=None):
    """eea_footprint_validate_control_batch: validate_control_batch for the polygon base fp -- valid int32 [P] = 1 when no step
    of the rollout of u [P][3] from x0 [P][3] collides; sq as in footprint_check_batch.  Device tensors; asynchronous"""
    check(lib().eea_footprint_validate_control_batch(device, C.byref(cfg), C.byref(fp), _ptr(grid), _ptr(sq), _ptr(x0), _ptr(u),
                                                     dt, horizon, int(x0.shape[0]), _ptr(valid), C.c_void_p(stream or 0)))


def footprint_dwa_control_batch(ccfg, dcfg, fp, grid, x0, vb, u_opt, found, sq=None, vref=None, xt_ref=None, dt_ref=0.0, device=0,
                                stream=None):
    """eea_footprint_dwa_control_batch: dwa_control_batch for the polygon base fp; sq as in footprint_check_batch.  Device
    tensors; asynchronous"""
    n_ref = xt_ref.shape[1] if xt_ref is not None else 0
    check(lib().eea_footprint_dwa_control_batch(device, C.byref(ccfg), C.byref(dcfg), C.byref(fp), _ptr(grid), _ptr(sq), _ptr(x0),
                                                _ptr(vb), _ptr(vref), _ptr(xt_ref), n_ref, dt_ref, int(x0.shape[0]), _ptr(u_opt),
                                                _ptr(found), C.c_void_p(stream or 0)))


def release_collision_caches():
    """drops the cached ring offsets / map buffers of the collision, validate, DWA and clearance calls"""
    L = lib()
    L.eea_release_collision_caches.restype = None
    L.eea_release_collision_caches()


def set_option(option, value):
    """eea_set_option: process-wide dispatch option (OPT_*)"""
    check(lib().eea_set_option(option, value))


def integrate_twist_batch(x0, u, dt, out=None, normalize_heading=False, stream=None, device=0):
    """eea_integrate_twist_batch (ABI 6): integrate_twist (numerics.hpp:273-297) of P poses on the device; out may be x0"""
    out = x0 if out is None else out
    lib().eea_integrate_twist_batch.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_uint, C.c_void_p, C.c_int, C.c_void_p]
    check(lib().eea_integrate_twist_batch(device, _ptr(x0), _ptr(u), float(dt), int(x0.shape[0]), _ptr(out),
                                          1 if normalize_heading else 0, C.c_void_p(stream or 0)))
    return out


def sense_ray_count(range_cells):
    """eea_sense_ray_count: rays per robot of eea_sense_reveal_batch, 8 * range_cells"""
    return int(lib().eea_sense_ray_count(int(range_cells)))


def sense_reveal_batch(cfg, range_cells, truth, known, pose, ranges=None, mask=None, device=0, stream=None):
    """eea_sense_reveal_batch: the P robots of pose [P][3] cast 8 * range_cells rays through the int8 grid truth; the cells
    they cross are copied into known (in place); ranges [P][8 * range_cells] int32 (optional) receives the step at which a ray
    met a blocking cell or -1; mask [P] int32 (optional): robots with 0 are left out.  Device tensors; asynchronous"""
    check(lib().eea_sense_reveal_batch(device, C.byref(cfg), int(range_cells), _ptr(truth), _ptr(known), _ptr(pose), _ptr(mask),
                                       int(pose.shape[0]), _ptr(ranges), C.c_void_p(stream or 0)))


def grid_census(cfg, grid, counts, device=0, stream=None):
    """eea_grid_census: counts [3] (device, 64-bit integers) = unknown cells (< 0), known cells below the occupied threshold,
    blocking cells of the int8 device grid; asynchronous"""
    check(lib().eea_grid_census(device, C.byref(cfg), _ptr(grid), _ptr(counts), C.c_void_p(stream or 0)))


def evidence_table(ecfg):
    """eea_evidence_table: int8 array of 2 e_clip + 1: entry e + e_clip is the occupancy probability (1 .. 99) eea_evidence_publish
    writes for e evidence units -- the bytes the device looks up.  Host only"""
    import numpy as np
    table = np.empty(2 * min(max(int(ecfg.e_clip), 0), 1024) + 1, dtype=np.int8)   # (an e_clip outside 1 .. 1024 is refused)
    check(lib().eea_evidence_table(C.byref(ecfg), table.ctypes.data_as(C.c_void_p)))
    return table


def sense_observe_batch(cfg, ecfg, range_cells, scan, truth, evid, pose, ranges=None, mask=None, robot0=0, device=0, stream=None):
    """eea_sense_observe_batch: one noisy scan (number `scan`) of the P robots of pose [P][3], robot b being robot0 + b of the
    fleet, through the int8 grid truth, fused into evid (int32 [ysize][xsize], in place: + w_occ on a touched cell that appears
    blocking, - w_free on every other touched cell); ranges [P][8 * range_cells] int32 (optional): the step at which a ray met a
    cell that appeared blocking or -1; mask [P] int32 (optional): robots with 0 are left out.  Device tensors; asynchronous"""
    check(lib().eea_sense_observe_batch(device, C.byref(cfg), C.byref(ecfg), int(range_cells), int(scan), int(robot0), _ptr(truth),
                                        _ptr(evid), _ptr(pose), _ptr(mask), int(pose.shape[0]), _ptr(ranges),
                                        C.c_void_p(stream or 0)))


def evidence_publish(cfg, ecfg, evid, known, counts=None, device=0, stream=None):
    """eea_evidence_publish: known (int8 [ysize][xsize], every element overwritten) = -1 where evid is 0, else the table's
    probability of the clamped evidence; counts [3] (device, 64-bit integers, optional): eea_grid_census of known; asynchronous"""
    check(lib().eea_evidence_publish(device, C.byref(cfg), C.byref(ecfg), _ptr(evid), _ptr(known), _ptr(counts),
                                     C.c_void_p(stream or 0)))


def sense_gain_field(cfg, range_cells, stride, known, gain, device=0, stream=None):
    """eea_sense_gain_field: gain (device uint32 [ysize][xsize], every element overwritten) = per candidate cell (both indices
    multiples of stride, the cell not blocking) the unknown cells the sensor's 8 * range_cells rays would cross from there
    through the int8 device grid `known`, counted per beam, + 1 for an unknown own cell; 0 elsewhere; asynchronous"""
    check(lib().eea_sense_gain_field(device, C.byref(cfg), int(range_cells), int(stride), _ptr(known), _ptr(gain),
                                     C.c_void_p(stream or 0)))


def sense_mi_table(cfg, p_unknown):
    """eea_sense_mi_table: (h, pass), two float64 arrays of 256: entry v + 128 holds h(v) / pass(v) of the int8 cell value v at
    cfg's occupied_threshold and the probability p_unknown of an unknown cell -- the doubles the field entries use.  Host only"""
    import numpy as np
    h, pass_ = np.empty(256, dtype=np.float64), np.empty(256, dtype=np.float64)
    check(lib().eea_sense_mi_table(C.byref(cfg), float(p_unknown), h.ctypes.data_as(C.c_void_p), pass_.ctypes.data_as(C.c_void_p)))
    return h, pass_


def sense_mi_field(cfg, range_cells, stride, known, mi, p_unknown=0.5, device=0, stream=None):
    """eea_sense_mi_field: mi (device double [ysize][xsize], every element overwritten) = per candidate cell (both indices
    multiples of stride, the cell not blocking) the Shannon mutual information between the map and the sensor's
    8 * range_cells ideal beams cast from there through the int8 device grid `known`; +0.0 elsewhere; asynchronous"""
    check(lib().eea_sense_mi_field(device, C.byref(cfg), int(range_cells), int(stride), float(p_unknown), _ptr(known), _ptr(mi),
                                   C.c_void_p(stream or 0)))


def stream_wait_flag(flag, seq, timeouts=None, stream=None):
    """eea_stream_wait_flag (ABI 6): what follows on `stream` starts once *flag - seq >= 0 -- a one-wavefront gate kernel"""
    check(lib().eea_stream_wait_flag(_ptr(flag), seq, _ptr(timeouts), C.c_void_p(stream or 0)))


def prepared_stream_wait_flag(flag, timeouts=None, stream=None):
    """a callable gate(seq) with the pointers converted once (a pass of 4096 agents takes ~23 us: per-pass host work counts)"""
    fn, f, t, s = lib().eea_stream_wait_flag, _ptr(flag), _ptr(timeouts), C.c_void_p(stream or 0)

    def gate(seq):
        check(fn(f, seq, t, s))
    return gate


def get_option(option):
    return lib().eea_get_option(option)


class FleetLayer:
    """eea_fleet_layer: the B robots of a fleet as obstacles to one another (include/ergodic_amd.h states the rule).  cfg: the
    make_collision_cfg(...) of the ticks that use it; body_cells: the body radius in cells (the natural value is the boundary
    radius in cells).  update() builds the layer from the poses on the stream; Engine.tick_batch_fleet / collision_check read it."""
    NOT_STAMPED = -2 ** 31

    def __init__(self, cfg, body_cells, B, device=0):
        self.h = C.c_void_p()
        check(lib().eea_fleet_layer_create(device, C.byref(cfg) if cfg is not None else None, int(body_cells), int(B), C.byref(self.h)))
        self.cfg, self.body_cells, self.B = cfg, int(body_cells), int(B)
        self.reach = int(lib().eea_fleet_layer_reach(self.h))
        self.shape = (cfg.ysize + 2 * self.reach, cfg.xsize + 2 * self.reach)   # of the counts: centres [-R', size + R')

    def update(self, pose, mask=None, stream=None):
        """pose [B][3] float64, mask [B] int32 or None: device tensors; asynchronous"""
        check(lib().eea_fleet_layer_update(self.h, _ptr(pose), _ptr(mask), C.c_void_p(stream or 0)))

    def read(self):
        """(counts [ysize + 2R'][xsize + 2R'], cells [B][2] as (x, y)) as numpy int32 arrays; synchronises"""
        import numpy as np
        count, cell = np.empty(self.shape, dtype=np.int32), np.empty((self.B, 2), dtype=np.int32)
        check(lib().eea_fleet_layer_read(self.h, _ptr(count), _ptr(cell)))
        return count, cell

    def collision_check(self, grid, pose, hit, self_index=None, stream=None):
        """eea_fleet_collision_check_batch: hit [P] int32 = collisionCheck of pose [P][3] on grid (None: robots only) OR a
        collision with a robot other than self_index [P] int32 (-1 / None: nobody's pose)"""
        check(lib().eea_fleet_collision_check_batch(self.h, _ptr(grid), _ptr(pose), _ptr(self_index), int(pose.shape[0]),
                                                    _ptr(hit), C.c_void_p(stream or 0)))

    def close(self):
        if self.h:
            lib().eea_fleet_layer_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


BODY_LAYER_NO_FILTER = 1   # EEA_BODY_LAYER_NO_FILTER


class BodyLayer:
    """eea_body_layer: the B robots of a fleet, each the convex polygon fp (a Footprint), as obstacles to one another
    (include/ergodic_amd.h states the rule).  cfg: the make_collision_cfg(...) of the grid -- the geometry and
    occupied_threshold are read.  update() builds the layer from the poses on the stream; check / validate / dwa and
    Engine.tick_batch_bodies read it.  self_index [P] int32: the robot each pose belongs to (-1 / None: nobody)"""
    SNAP = 5    # doubles per snapshot record: px, py, sine, cosine, stamped

    def __init__(self, cfg, fp, B, flags=0, device=0):
        self.h = C.c_void_p()
        check(lib().eea_body_layer_create(device, C.byref(cfg) if cfg is not None else None, C.byref(fp) if fp is not None else None,
                                          int(B), int(flags), C.byref(self.h)))
        self.cfg, self.fp, self.B, self.flags = cfg, fp, int(B), int(flags)
        self.box = int(lib().eea_body_layer_box(self.h))
        self.cover_shape = (cfg.ysize, cfg.xsize)
        self.near_shape = (cfg.ysize + 2 * self.box, cfg.xsize + 2 * self.box)   # the cells [-box, size + box)

    def update(self, pose, mask=None, stream=None):
        """pose [B][3] float64, mask [B] int32 or None: device tensors; asynchronous"""
        check(lib().eea_body_layer_update(self.h, _ptr(pose), _ptr(mask), C.c_void_p(stream or 0)))

    def read(self):
        """(cover [ysize][xsize], near [ysize + 2 box][xsize + 2 box], snapshot [B][5]) as numpy arrays; synchronises"""
        import numpy as np
        cover, near = np.empty(self.cover_shape, dtype=np.int32), np.empty(self.near_shape, dtype=np.int32)
        snap = np.empty((self.B, self.SNAP), dtype=np.float64)
        check(lib().eea_body_layer_read(self.h, _ptr(cover), _ptr(near), _ptr(snap)))
        return cover, near, snap

    def check(self, grid, pose, hit, sq=None, self_index=None, stream=None):
        """eea_body_collision_check_batch: hit [P] int32 = the footprint's verdict of pose [P][3] on grid (None: robots only)
        OR a shared cell with the body of a robot other than self_index"""
        check(lib().eea_body_collision_check_batch(self.h, _ptr(grid), _ptr(sq), _ptr(pose), _ptr(self_index),
                                                   int(pose.shape[0]) if pose is not None else 0, _ptr(hit),
                                                   C.c_void_p(stream or 0)))

    def validate(self, grid, x0, u, dt, horizon, valid, sq=None, self_index=None, stream=None):
        """eea_body_validate_control_batch: footprint_validate_control_batch with the layer"""
        check(lib().eea_body_validate_control_batch(self.h, _ptr(grid), _ptr(sq), _ptr(x0), _ptr(u), _ptr(self_index), dt, horizon,
                                                    int(x0.shape[0]) if x0 is not None else 0, _ptr(valid),
                                                    C.c_void_p(stream or 0)))

    def dwa(self, dcfg, grid, x0, vb, u_opt, found, sq=None, vref=None, xt_ref=None, dt_ref=0.0, self_index=None, stream=None):
        """eea_body_dwa_control_batch: footprint_dwa_control_batch with the layer"""
        n_ref = xt_ref.shape[1] if xt_ref is not None else 0
        check(lib().eea_body_dwa_control_batch(self.h, C.byref(dcfg) if dcfg is not None else None, _ptr(grid), _ptr(sq), _ptr(x0),
                                               _ptr(vb), _ptr(vref), _ptr(xt_ref), n_ref, dt_ref, _ptr(self_index),
                                               int(x0.shape[0]) if x0 is not None else 0, _ptr(u_opt), _ptr(found),
                                               C.c_void_p(stream or 0)))

    def close(self):
        if self.h:
            lib().eea_body_layer_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ReplayMemory:
    """eea_replay: the replay memory of a fleet in device memory -- ReplayBuffer::append / sampleMemory (buffer.cpp) for B robots
    as kernels that fill the mem_cols / n_mem tensors control_batch / tick_batch take.  Poses and columns are device tensors of
    the dtype real_size names (8: float64, 4: float32), masks and n_mem int32; `draw` is the caller's tick counter (a draw is a
    pure function of (seed, draw, robot0 + b, column): ergodic_amd.h)."""

    def __init__(self, B, capacity, batch_size, seed=0, robot0=0, real_size=8, device=0):
        self.h = C.c_void_p()
        check(lib().eea_replay_create(device, B, capacity, batch_size, seed, robot0, real_size, C.byref(self.h)))
        self.B, self.capacity, self.batch_size, self.real_size = B, capacity, batch_size, real_size
        self._coverage_ws = None   # workspaces of coverage(): allocated once per object (and engine), not per call
        self._field_ws = {}        # ... and of coverage_fields(): per kind

    def append(self, pose, mask=None, stream=None):
        check(lib().eea_replay_append(self.h, _ptr(pose), _ptr(mask), C.c_void_p(stream or 0)))

    def sample(self, draw, mem_cols, n_mem, mem_stride=None, stream=None):
        stride = mem_cols.shape[1] if mem_stride is None else mem_stride
        check(lib().eea_replay_sample(self.h, draw, _ptr(mem_cols), _ptr(n_mem), stride, C.c_void_p(stream or 0)))

    def append_sample(self, pose, draw, mem_cols, n_mem, mask=None, mem_stride=None, stream=None):
        """the per-tick form, one launch: append, then sample from the memory that includes the new pose"""
        stride = mem_cols.shape[1] if mem_stride is None else mem_stride
        check(lib().eea_replay_append_sample(self.h, _ptr(pose), _ptr(mask), draw, _ptr(mem_cols), _ptr(n_mem), stride,
                                             C.c_void_p(stream or 0)))

    def prepared_append_sample(self, pose, mem_cols, n_mem, mask=None, stream=None):
        """a callable tick(draw) with the pointers converted once (the launch is a few microseconds: per-tick host work counts)"""
        fn, h = lib().eea_replay_append_sample, self.h
        a = (_ptr(pose), _ptr(mask), _ptr(mem_cols), _ptr(n_mem), mem_cols.shape[1], C.c_void_p(stream or 0))
        keep = (pose, mask, mem_cols, n_mem)

        def call(draw, _keep=keep):
            rc = fn(h, a[0], a[1], draw, a[2], a[3], a[4], a[5])
            if rc != 0:
                check(rc)
        return call

    def sample_pool(self, draw, n_cols, mem_cols, n_mem, exclude_self=False, accumulate=False, mem_stride=None, stream=None):
        """eea_replay_pool_sample: up to n_cols columns per robot from the pooled history of ALL robots of this object
        (exclude_self: without the robot's own poses); accumulate: behind the n_mem[b] columns the row already holds (after
        sample / append_sample on the same stream), clipped at the stride; asynchronous, two launches"""
        stride = mem_cols.shape[1] if mem_stride is None else mem_stride
        check(lib().eea_replay_pool_sample(self.h, draw, n_cols, 1 if exclude_self else 0, 1 if accumulate else 0, _ptr(mem_cols),
                                           _ptr(n_mem), stride, C.c_void_p(stream or 0)))

    def counts(self):
        """(poses stored per robot [B], appends dropped by full stores in total); waits for the device"""
        import numpy as np
        n, dropped = np.empty(self.B, dtype=np.uint32), C.c_ulonglong(0)
        check(lib().eea_replay_counts(self.h, _ptr(n), C.byref(dropped)))
        return n, int(dropped.value)

    def read(self, b, first=0, n=None):
        """poses first .. first + n - 1 of robot b as a host array [n][3] (n = None: up to the robot's count); waits for the device"""
        import numpy as np
        if n is None:
            n = int(self.counts()[0][b]) - first
        out = np.empty((n, 3), dtype=np.float64 if self.real_size == 8 else np.float32)
        check(lib().eea_replay_read(self.h, b, first, n, _ptr(out)))
        return out

    def reset(self, stream=None):
        check(lib().eea_replay_reset(self.h, C.c_void_p(stream or 0)))

    def history_records(self, engine, out, stream=None):
        """eea_replay_history_records: out [B][engine.ck_record_len] = the sum record of every robot's whole stored history
        (sum over its poses of the K^2 basis products in the engine's current domain; element K^2 = its count); asynchronous"""
        check(lib().eea_replay_history_records(engine.h, self.h, _ptr(out), C.c_void_p(stream or 0)))

    def coverage(self, engine, stream=None):
        """(eps per robot [B], eps of the fleet [1]) as device tensors: the ergodic metric sum_k lamda_k (c_k - phi_k)^2 of each
        robot's whole stored history and of all of them together -- history_records, eea_ck_records_sum over the B rows,
        records_metric on both; asynchronous on `stream`, no host round trip.  The tensors (and the per-robot / fleet records
        in self.coverage_records) belong to this object and are overwritten by the next call for the same engine."""
        import torch
        ws = self._coverage_ws
        if ws is None or ws[0] is not engine:
            dt, L = torch.float64 if self.real_size == 8 else torch.float32, engine.ck_record_len
            new = lambda *shape: torch.empty(shape, dtype=dt, device="cuda")   # (every element is written by the kernels)
            ws = self._coverage_ws = (engine, new(self.B, L), new(L), new(self.B), new(1))
        _, rec, fleet, eps, eps_fleet = ws
        self.history_records(engine, rec, stream)
        engine.ck_records_sum(self.B, rec, fleet, stream)
        records_metric(engine, rec, eps, stream=stream)
        records_metric(engine, fleet, eps_fleet, stream=stream)
        return eps, eps_fleet

    @property
    def coverage_records(self):
        """(per-robot sum records [B][record_len], fleet sum record [record_len]) of the last coverage() call"""
        return self._coverage_ws[1], self._coverage_ws[2]

    def coverage_fields(self, engine, kind, fleet_only=True, stream=None):
        """(fields per robot [B][ny][nx] -- None with fleet_only --, field of the fleet [ny][nx]) on the engine's target grid:
        records_field of `kind` (FIELD_*) on the records the last coverage(engine) call left in coverage_records; asynchronous
        on `stream`, no host round trip.  The tensors belong to this object, one set per kind, and are overwritten by the next
        call for that kind; the per-robot tensor is only allocated when asked for."""
        import torch
        cov = self._coverage_ws
        if cov is None or cov[0] is not engine:
            raise EngineError(ERR_INVALID_ARGUMENT, "coverage_fields: call coverage() with this engine first")
        nx, ny = engine.target_grid_size
        ws = self._field_ws.get(kind)
        if ws is None or ws[0] is not engine or ws[1] != (nx, ny):
            ws = self._field_ws[kind] = [engine, (nx, ny), None, torch.empty((ny, nx), dtype=cov[1].dtype, device="cuda")]
        if not fleet_only:
            if ws[2] is None:
                ws[2] = torch.empty((self.B, ny, nx), dtype=cov[1].dtype, device="cuda")
            records_field(engine, kind, cov[1], ws[2], nx, ny, stream=stream)
        records_field(engine, kind, cov[2], ws[3], nx, ny, stream=stream)
        return (None if fleet_only else ws[2]), ws[3]

    def close(self):
        self._coverage_ws = None
        self._field_ws = {}
        if self.h:
            lib().eea_replay_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def records_metric(engine, rec, metric, ck=None, stream=None):
    """eea_records_metric: metric[j] = sum_m lamda_m (rec[j][m] / rec[j][K^2] - phi_m)^2 for the sum records rec
    [n][engine.ck_record_len] (or one record [record_len]); ck [n][K^2] (optional) receives the quotients; asynchronous"""
    n = 1 if rec.dim() == 1 else int(rec.shape[0])
    check(lib().eea_records_metric(engine.h, n, _ptr(rec), _ptr(metric), _ptr(ck), C.c_void_p(stream or 0)))


def records_field(engine, kind, rec, out, nx=None, ny=None, row0=0, nrows=None, stream=None):
    """eea_records_field: out [n][nrows][nx] = the field `kind` (FIELD_DENSITY / FIELD_DEFICIT / FIELD_POTENTIAL) of the sum
    records rec [n][engine.ck_record_len] (or one record [record_len]) on the rows row0 .. row0 + nrows - 1 of an nx x ny grid
    (default: the engine's target grid, all rows); asynchronous"""
    n = 1 if rec.dim() == 1 else int(rec.shape[0])
    if nx is None or ny is None:
        gx, gy = engine.target_grid_size
        nx, ny = (gx if nx is None else nx), (gy if ny is None else ny)
    if nrows is None:
        nrows = max(ny - row0, 0)
    check(lib().eea_records_field(engine.h, kind, n, _ptr(rec), nx, ny, row0, nrows, _ptr(out), C.c_void_p(stream or 0)))


COMM_ID_BYTES = 128


def comm_set_library(path):
    """binds the collectives to the RCCL at `path` (process-wide, before the first other comm call): eea_comm_set_library"""
    check(lib().eea_comm_set_library(os.fsencode(path)))


def comm_unique_id():
    """128-byte RCCL id created on this rank (rank 0 hands it to the others)"""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    check(lib().eea_comm_get_unique_id(buf))
    return buf.raw


class ConsensusPlan:
    """eea_consensus_plan (ABI 6): `passes_per_launch` consensus passes of a rank -- per pass and agent group one control launch
    (records out, the sum record of pass i - lag in), the record sum and the all-reduce over the ranks -- as ONE replayable
    device graph.  groups: a list of dicts with B, pose, ut, u0 and optionally mem_cols, n_mem, mem_stride, status, skip
    (device tensors; the plan keeps them alive)."""

    def __init__(self, eng, comm, groups, lag=2, passes_per_launch=48):
        self.h = C.c_void_p()
        self._keep = list(groups)
        n = len(groups)
        agents = (C.c_uint * n)(*[int(g["B"]) for g in groups])
        ios = (BatchIO * n)()
        for io, g in zip(ios, groups):
            io.d_pose, io.d_ut, io.d_u0 = _ptr(g["pose"]), _ptr(g["ut"]), _ptr(g["u0"])
            io.d_mem_cols, io.d_n_mem, io.mem_stride = _ptr(g.get("mem_cols")), _ptr(g.get("n_mem")), int(g.get("mem_stride", 0) or 0)
            io.d_status, io.d_skip = _ptr(g.get("status")), _ptr(g.get("skip"))
        d = ConsensusDesc(n, agents, ios, lag, passes_per_launch)
        check(lib().eea_consensus_plan_create(eng.h, comm.h, C.byref(d), C.byref(self.h)))
        passes, last = C.c_uint(), C.c_void_p()
        check(lib().eea_consensus_plan_info(self.h, C.byref(passes), C.byref(last)))
        self.passes_per_launch, self.d_last_sum = passes.value, last.value
        self._launch = lib().eea_consensus_plan_launch

    def launch(self, stream=None):
        check(self._launch(self.h, C.c_void_p(stream or 0)))

    def last_sum(self, eng):
        """the sum record the last pass of a launch leaves, as a host array [eea_ck_record_len] (synchronise first)"""
        import numpy as np
        n = eng.ck_record_len
        out = np.empty(n, dtype=np.float32 if eng.real_size == 4 else np.float64)
        hip = C.CDLL("libamdhip64.so")   # (already mapped: the library links it)
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        if hip.hipMemcpy(out.ctypes.data, self.d_last_sum, out.nbytes, 2) != 0:   # hipMemcpyDeviceToHost
            raise EngineError(ERR_HIP, "hipMemcpy of the plan's sum record failed")
        return out

    def close(self):
        if self.h:
            lib().eea_consensus_plan_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """Communicator of the agent-batch exchange steps (RCCL over xGMI; ncclComm behind the C ABI).
    uid=None with nranks == 1: local communicator without RCCL."""

    def __init__(self, device, nranks, rank, uid=None):
        self.h = C.c_void_p()
        idbuf = C.create_string_buffer(uid, COMM_ID_BYTES) if uid is not None else None
        check(lib().eea_comm_create(device, nranks, rank, idbuf, C.byref(self.h)))
        self.nranks, self.rank = nranks, rank

    def close(self):
        if self.h:
            lib().eea_comm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def library_nranks(self):
        """ncclCommCount of the communicator behind the C ABI (0: local communicator, -1: the library cannot tell)"""
        lib().eea_comm_library_nranks.argtypes = [C.c_void_p]
        return int(lib().eea_comm_library_nranks(self.h))

    def allgather_ck(self, eng, B_local, ck_local, ck_all, stream=None):
        check(lib().eea_comm_allgather_ck(eng.h, self.h, B_local, _ptr(ck_local), _ptr(ck_all),
                                          C.c_void_p(stream or 0)))

    def consensus_ck(self, eng, B_local, ck_local, ck_shared, stream=None):
        check(lib().eea_comm_consensus_ck(eng.h, self.h, B_local, _ptr(ck_local), _ptr(ck_shared),
                                          C.c_void_p(stream or 0)))

    def consensus_ck_async(self, eng, B_local, ck_local, ck_shared, compute_stream, slot):
        check(lib().eea_comm_consensus_ck_async(eng.h, self.h, B_local, _ptr(ck_local), _ptr(ck_shared),
                                                C.c_void_p(compute_stream or 0), slot))

    def allgather_ck_async(self, eng, B_local, ck_local, ck_all, compute_stream, slot):
        check(lib().eea_comm_allgather_ck_async(eng.h, self.h, B_local, _ptr(ck_local), _ptr(ck_all),
                                                C.c_void_p(compute_stream or 0), slot))

    def wait(self, slot, stream=None):
        check(lib().eea_comm_wait(self.h, slot, C.c_void_p(stream or 0)))

    def records_exchange_async(self, eng, B_local, ck_rec, out_sum, group_streams, slot):
        """eea_comm_records_exchange_async: record sum + all-reduce on the communicator's stream, after every group stream"""
        arr = (C.c_void_p * len(group_streams))(*[C.c_void_p(s or 0) for s in group_streams])
        check(lib().eea_comm_records_exchange_async(eng.h, self.h, B_local, _ptr(ck_rec), _ptr(out_sum), arr,
                                                    len(group_streams), slot))

    def prepared_records_exchange(self, eng, B_local, ck_rec, out_sum, group_streams, slot):
        """the same as a callable with the argument marshalling done once (bench.py's per-pass call)"""
        arr = (C.c_void_p * len(group_streams))(*[C.c_void_p(s or 0) for s in group_streams])
        fn, args = lib().eea_comm_records_exchange_async, (eng.h, self.h, B_local, _ptr(ck_rec), _ptr(out_sum), arr,
                                                           len(group_streams), slot)
        keep = (ck_rec, out_sum, arr)

        def call(_keep=keep):
            rc = fn(*args)
            if rc != 0:
                check(rc)
        return call

    def records_exchange_bound(self, eng, B_local, ck_rec, rec_ready, seq, out_sum, flag, slot):
        """eea_comm_records_exchange_bound: the device-bound exchange of one pass (no host or stream waits anywhere)"""
        check(lib().eea_comm_records_exchange_bound(eng.h, self.h, B_local, _ptr(ck_rec), _ptr(rec_ready), seq,
                                                    _ptr(out_sum), _ptr(flag), slot))

    def prepared_records_exchange_bound(self, eng, B_local, ck_rec, rec_ready, out_sum, flag, slot):
        """the same as a callable call(seq) with the argument marshalling done once"""
        fn, h, eh = lib().eea_comm_records_exchange_bound, self.h, eng.h
        a = (_ptr(ck_rec), _ptr(rec_ready), _ptr(out_sum), _ptr(flag))
        keep = (ck_rec, rec_ready, out_sum, flag)

        def call(seq, _keep=keep):
            rc = fn(eh, h, B_local, a[0], a[1], seq, a[2], a[3], slot)
            if rc != 0:
                check(rc)
        return call

    def prepared_wait(self, slot, stream):
        fn, args = lib().eea_comm_wait, (self.h, slot, C.c_void_p(stream or 0))

        def call():
            rc = fn(*args)
            if rc != 0:
                check(rc)
        return call

    def allreduce_sum_async(self, eng, buf, n, compute_stream, slot):
        check(lib().eea_comm_allreduce_sum_async(eng.h, self.h, _ptr(buf), n, C.c_void_p(compute_stream or 0), slot))

    def allreduce_sum(self, eng, buf, n, stream=None):
        check(lib().eea_comm_allreduce_sum(eng.h, self.h, _ptr(buf), n, C.c_void_p(stream or 0)))
