"""Host-side mirror of the reference's interfaces on top of libqrgpu.so (ctypes).

Reference interface                                   -> here
  Quadruped::SetupProblem / SolveMPCKernel / GetMPCSolution
      (QI/controllers/mpc/qr_mpc_interface.h:157,200,215) -> MPCInterface.SetupProblem / SolveMPCKernel / GetMPCSolution
  qrWbcLocomotionController<float>::Run
      (QI/controllers/wbc/qr_wbc_locomotion_controller.hpp:59) -> WbcLocomotionController.Run
  batched ticks (no reference equivalent; n independent robots) -> Context.mpc_solve_batch / wbc_run_batch / tick_batch

There is no CPU path in this module: if the HIP library is missing or no gfx950 device is
usable, construction raises (MissingExtension / QrgpuError).  torch is used only by callers
for device memory, streams and torch.distributed; this module takes raw device pointers
(ints) or anything with a .data_ptr() method.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

ERRORS = {0: "OK", 1: "NO_DEVICE", 2: "BAD_ARG", 3: "NOT_SETUP", 4: "LAUNCH", 5: "ALLOC", 6: "COMM"}
ST_FLAG_MASK, ST_BAD_TYPE = 0xff0000ff, 0x01000000

ST_MPC_MAXITER, ST_MPC_INFEAS, ST_MPC_OVERFLOW, ST_MPC_NOTSPD = 0x1, 0x2, 0x4, 0x8
ST_WBC_MAXITER, ST_WBC_INFEAS = 0x10, 0x20
GAIT_RESET_CONSTRUCT, GAIT_RESET_LIVE = 1, 2          # qrgpu_gait_update_batch's reset (include/qrgpu.h)
MAX_GAITS, GAIT_BAD_SEL = 8, 0x1                      # qrgpu_gait_select_update_batch: the table's capacity, the bit of gait_flags
FB_DEBUG_FLOATS = 324 + 18 + 18 + 216 + 12 + 12 + 12


def status_flags(status):
    """Flag bits of a status word / array (include/qrgpu.h: bits 0-7 and 24-31; 0 = converged)."""
    return np.asarray(status).astype(np.int64) & ST_FLAG_MASK


def status_iterations(status):
    """MPC active-set iteration count of a status word / array (bits 8-23)."""
    return (np.asarray(status).astype(np.int64) >> 8) & 0xffff


class QrgpuError(RuntimeError):
    pass


class MissingExtension(QrgpuError):
    """libqrgpu.so has not been built (run `python -c 'import __graft_entry__ as g; g.build()'`)."""


def _set_fields(d, fields):
    """Set fields of a ctypes struct from a dict: scalars or sequences by name, None = leave as it is.  Whether a value becomes an int or a
    float is decided by the field's ctype."""
    ctype_of = dict(d._fields_)
    for name, v in fields.items():
        if v is None:
            continue
        if name not in ctype_of:
            raise AttributeError("%s has no field %r" % (type(d).__name__, name))
        t = ctype_of[name]
        if issubclass(t, C.Array):
            conv = int if issubclass(t._type_, (C.c_int, C.c_uint)) else float
            arr = getattr(d, name)
            for k, x in enumerate(v): arr[k] = conv(x)
        else:
            setattr(d, name, (int if issubclass(t, (C.c_int, C.c_uint)) else float)(v))
    return d


class model_desc_struct(C.Structure):
    _fields_ = [("hip_l", C.c_float), ("upper_l", C.c_float), ("lower_l", C.c_float), ("body_size", C.c_float * 3),
                ("kp_body_pos", C.c_float), ("kd_body_pos", C.c_float), ("kp_body_ori", C.c_float), ("kd_body_ori", C.c_float),
                ("kp_foot", C.c_float), ("kd_foot", C.c_float), ("weight_fb", C.c_float), ("weight_fr", C.c_float), ("mu", C.c_float)]


class vmc_desc_struct(C.Structure):
    _fields_ = [("mass", C.c_float), ("inertia", C.c_float * 9), ("acc_weight", C.c_float * 6), ("reg_weight", C.c_float),
                ("friction", C.c_float), ("fmin_ratio", C.c_float), ("fmax_ratio", C.c_float),
                ("hip_l", C.c_float), ("upper_l", C.c_float), ("lower_l", C.c_float)]


class estimator_desc_struct(C.Structure):
    _fields_ = [("hip_l", C.c_float), ("upper_l", C.c_float), ("lower_l", C.c_float), ("hip_offset", C.c_float * 12),
                ("time_step", C.c_float), ("accelerometer_variance", C.c_float), ("sensor_variance", C.c_float), ("window", C.c_int),
                ("body_height", C.c_float)]


def _estimator_desc(cfg20, geometry_only=False):
    """qrgpu_estimator_desc from workload.estimator_cfg() (an estimator_desc_struct is passed on as it is).  geometry_only: the leg geometry
    alone -- hip_l, upper_l, lower_l, hip_offset -- and the rest zero: all the swing stages read."""
    if isinstance(cfg20, estimator_desc_struct):
        return cfg20
    v = np.asarray(cfg20, np.float32)
    d = _set_fields(estimator_desc_struct(), dict(hip_l=v[0], upper_l=v[1], lower_l=v[2], hip_offset=v[7:19]))
    if not geometry_only:
        _set_fields(d, dict(time_step=v[3], accelerometer_variance=v[4], sensor_variance=v[5], window=v[6], body_height=v[19]))
    return d


class foothold_desc_struct(C.Structure):
    _fields_ = [("hip_offset", C.c_float * 12), ("default_hip_position", C.c_float * 12), ("hip_l", C.c_float), ("swing_kp", C.c_float * 3),
                ("foot_clearance", C.c_float)]


class gait_desc_struct(C.Structure):
    _fields_ = [("stance_duration", C.c_float * 4), ("duty_factor", C.c_float * 4), ("initial_leg_phase", C.c_float * 4),
                ("initial_leg_state", C.c_int * 4), ("contact_detection_phase_threshold", C.c_float), ("wait_time", C.c_float),
                ("advanced_trot", C.c_int)]


class walk_gait_desc_struct(C.Structure):
    _fields_ = [("stance_duration", C.c_float * 4), ("duty_factor", C.c_float * 4), ("initial_leg_phase", C.c_float * 4),
                ("initial_leg_state", C.c_int * 4), ("contact_detection_phase_threshold", C.c_float), ("n_states", C.c_int),
                ("state_switch", C.c_int * 4), ("state_ratio", C.c_float * 4)]


class swing_velocity_desc_struct(C.Structure):
    _fields_ = [("hip_position_com", C.c_float * 12), ("stance_duration", C.c_float * 4), ("swing_kp", C.c_float * 3), ("desired_height", C.c_float)]


MAX_GAPS = 8
SWING_MAX_PLAN = 32
SWING_STATE_FLOATS = 105 + 4 * SWING_MAX_PLAN
SWING_OUT_ROWS = 52
MODE_VELOCITY, MODE_POSITION, MODE_WALK, MODE_ADVANCED_TROT = 0, 1, 2, 3
SW_NO_TRAJECTORY, SW_PHASE_RANGE, SW_PLAN_EXIT, SW_PLAN_EMPTY, SW_PLAN_FULL = 0x1, 0x2, 0x4, 0x8, 0x10


class swing_mode_desc_struct(C.Structure):
    _fields_ = [("mode", C.c_int), ("terrain", C.c_int), ("is_sim", C.c_int), ("foothold_delta", C.c_float), ("n_gaps", C.c_int),
                ("gap_distance", C.c_float * MAX_GAPS), ("gap_width", C.c_float)]


def swing_mode_desc(mode, terrain=None, is_sim=None, foothold_delta=None, gaps=None, gap_width=None):
    """qrgpu_swing_mode_desc: the library's defaults for `mode` (config/a1_sim), with any field overridden."""
    d = swing_mode_desc_struct()
    load_library().qrgpu_swing_mode_desc_default(C.byref(d), int(mode))
    _set_fields(d, dict(terrain=terrain, is_sim=None if is_sim is None else bool(is_sim), foothold_delta=foothold_delta, gap_width=gap_width))
    if gaps is not None:
        _set_fields(d, dict(n_gaps=len(gaps), gap_distance=list(gaps)[:MAX_GAPS]))
    return d


STANCE_CMD_ROWS, STANCE_STATE_FLOATS, STANCE_OUT_ROWS, MOTOR_CMD_ROWS = 28, 1, 33, 60


class stance_desc_struct(C.Structure):
    _fields_ = [("mode", C.c_int), ("terrain", C.c_int), ("force_in_world", C.c_int), ("kp", C.c_float * 6), ("kd", C.c_float * 6),
                ("max_ddq", C.c_float * 6), ("min_ddq", C.c_float * 6), ("desired_height", C.c_float), ("desired_speed", C.c_float * 3),
                ("desired_twisting_speed", C.c_float), ("body_height", C.c_float), ("pose_reset_time", C.c_float),
                ("motor_kp", C.c_float * 12), ("motor_kd", C.c_float * 12)]


def stance_desc(mode, terrain=None, force_in_world=None, **fields):
    """qrgpu_stance_desc: the library's defaults for `mode` (config/a1_sim), with any field overridden (scalars or sequences by name)."""
    d = stance_desc_struct()
    load_library().qrgpu_stance_desc_default(C.byref(d), int(mode))
    _set_fields(d, dict(terrain=terrain, force_in_world=None if force_in_world is None else bool(force_in_world)))
    return _set_fields(d, fields)


POSE_MAX_LOOPS, POSE_STATE_ROWS = 20, 26
POSE_OUT_ROWS = 7 * POSE_MAX_LOOPS + 38
PP_FEW_CONTACTS, PP_NOT_PD, PP_INFEASIBLE, PP_LAMBDA_GROWN, PP_NONCONVEX, PP_NAN, PP_MAXITER = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40
POSE_EVENT_NONE, POSE_EVENT_UPDATE, POSE_EVENT_RESET_BASE_POSE, POSE_EVENT_SWITCH_TO_SWING = 0, 1, 2, 3


class pose_plan_desc_struct(C.Structure):
    _fields_ = [("rBH", C.c_float * 12), ("l_min", C.c_float), ("l_max", C.c_float), ("omega", C.c_float), ("eps", C.c_float),
                ("body_height", C.c_float), ("loops", C.c_int)]


def pose_plan_desc(**fields):
    """qrgpu_pose_plan_desc: the library's defaults (the reference's constants), with any field overridden (scalars or sequences by name)."""
    d = pose_plan_desc_struct()
    load_library().qrgpu_pose_plan_desc_default(C.byref(d))
    return _set_fields(d, fields)


PLANT_OUT_ROWS = 58
PL_NONFINITE, PL_QUAT_ZERO, PL_BAD_TYPE = 0x1, 0x2, 0x01000000


class plant_params_struct(C.Structure):
    _fields_ = [("dt", C.c_float), ("substeps", C.c_int), ("contact_k", C.c_float), ("contact_a", C.c_float), ("mu", C.c_float), ("v_eps", C.c_float),
                ("ground_z", C.c_float), ("tau_max", C.c_float), ("contact_threshold", C.c_float), ("com_offset", C.c_float * 3)]


def plant_params(**fields):
    """qrgpu_plant_params: the library's defaults (A1, 2 ms ticks of 2 sub-steps), with any field overridden (scalars or sequences by name)."""
    d = plant_params_struct()
    load_library().qrgpu_plant_params_default(C.byref(d))
    return _set_fields(d, fields)


TERRAIN_OUT_ROWS = 16
PL_BAD_FIELD, PL_OFF_FIELD = 0x4, 0x8


class terrain_desc_struct(C.Structure):
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("n_fields", C.c_int), ("x0", C.c_float), ("y0", C.c_float), ("cell", C.c_float)]


def terrain_desc(nx, ny, n_fields=1, x0=0.0, y0=0.0, cell=0.1):
    """qrgpu_terrain_desc: n_fields grids of ny x nx heights, x fastest; node (i, j) lies at (x0 + i cell, y0 + j cell)."""
    return terrain_desc_struct(int(nx), int(ny), int(n_fields), float(x0), float(y0), float(cell))


BODY_OUT_ROWS = 36
PL_TRUNK_CONTACT, PL_KNEE_CONTACT, PL_JOINT_LIMIT = 0x10, 0x20, 0x40


class plant_body_desc_struct(C.Structure):
    _fields_ = [("trunk_half", C.c_float * 3), ("trunk_center", C.c_float * 3), ("q_lo", C.c_float * 3), ("q_hi", C.c_float * 3), ("limit_k", C.c_float),
                ("limit_a", C.c_float)]


# What differs from the library's default (A1) per robot.  Lite3: the trunk's collision box 0.234 x 0.184 x 0.08 and the joint limits of
# lite3_description (HipX +-0.523, HipY -2.67..0.314, Knee 0.524..2.792) mapped into this library's sign convention, in which hip and knee turn the
# other way (the stand pose is 0, 0.8, -1.6; that description's knee is positive): lo = -upper, hi = -lower.
PLANT_BODY = {"a1": {}, "lite3": dict(trunk_half=(0.117, 0.092, 0.04), q_lo=(-0.523, -0.314, -2.792), q_hi=(0.523, 2.67, -0.524))}


def plant_body_desc(robot="a1", **fields):
    """qrgpu_plant_body_desc of "a1" (the library's default) or "lite3": trunk box, joint limits, the stops' stiffness and damping, with any field
    overridden (scalars or sequences by name)."""
    d = plant_body_desc_struct()
    load_library().qrgpu_plant_body_desc_default(C.byref(d))
    return _set_fields(_set_fields(d, PLANT_BODY[robot]), fields)


EP_STATUS, EP_TICK_STATUS, EP_NONFINITE, EP_TILT, EP_HEIGHT, EP_OFF_FIELD, EP_TIMEOUT, EP_FORCED = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80
EP_REASONS, EP_BAD_FIELD = 0xff, 0x01000000
EPISODE_STATE_ROWS, EPISODE_STATS_ROWS = 6, 9


class episode_desc_struct(C.Structure):
    _fields_ = [("status_mask", C.c_int), ("status_ticks", C.c_int), ("tick_mask", C.c_int), ("max_ticks", C.c_int), ("seed", C.c_uint),
                ("align_to_slope", C.c_int), ("tilt_max", C.c_float), ("min_clearance", C.c_float), ("field_margin", C.c_float),
                ("spawn_height", C.c_float), ("xy_jitter", C.c_float), ("yaw_jitter", C.c_float), ("q_jitter", C.c_float), ("v_jitter", C.c_float),
                ("q_spawn", C.c_float * 12), ("kp", C.c_float), ("kd", C.c_float)]


def episode_desc(**fields):
    """qrgpu_episode_desc: the library's defaults (a fall is PL_NONFINITE | PL_QUAT_ZERO | PL_TRUNK_CONTACT for one call, a tilt beyond 1 rad or a
    clearance under 0.10 m; spawn 0.30 above the ground at the stand pose, no jitter, no timeout, seed 1), with any field overridden."""
    d = episode_desc_struct()
    load_library().qrgpu_episode_desc_default(C.byref(d))
    return _set_fields(d, fields)


STAGE_RESET_CONSTRUCT, STAGE_RESET_LIVE = 1, 2


class stage_reset_struct(C.Structure):
    _fields_ = [("d_mask", C.c_void_p), ("bits", C.c_uint), ("level", C.c_int), ("d_ticks", C.c_void_p), ("tick_dt", C.c_float)]


def stage_reset(mask=None, bits=EP_REASONS, level=STAGE_RESET_CONSTRUCT, ticks=None, tick_dt=0.002):
    """qrgpu_stage_reset: mask [n] int32 on the device (robot r is reset at a stage call when (mask[r] & bits) != 0; e.g. the episode step's `done`),
    level STAGE_RESET_CONSTRUCT / STAGE_RESET_LIVE, ticks [n] int32 on the device (current_time_r = float32(ticks[r]) * tick_dt; e.g. row 0 of
    ep_state).  Either array may be None, not both."""
    d = stage_reset_struct()
    d.d_mask = None if mask is None else _dp(mask).value; d.bits = int(bits); d.level = int(level)
    d.d_ticks = None if ticks is None else _dp(ticks).value; d.tick_dt = float(tick_dt)
    return d


OBS_SIM, OBS_HARDWARE = 0, 1
OBSERVE_STATE_ROWS, OBSERVE_STATE_ROWS_MV = 71, 337


class observe_desc_struct(C.Structure):
    _fields_ = [("filter_rpy", C.c_int), ("filter_motor_velocity", C.c_int), ("yaw_offset", C.c_float), ("hip_l", C.c_float), ("upper_l", C.c_float),
                ("lower_l", C.c_float), ("hip_offset", C.c_float * 12), ("base_height", C.c_float), ("tick_ms", C.c_uint), ("seed", C.c_uint),
                ("acc_noise", C.c_float), ("gyro_noise", C.c_float), ("q_noise", C.c_float), ("qd_noise", C.c_float)]


def observe_desc(variant="sim", **fields):
    """qrgpu_observe_desc of the "sim" classes (rpy filter on, motor velocities as read) or the "hardware" class (rpy as read, motor velocities through
    the window of 20): A1's geometry, base height 0.27, 2 ms ticks, seed 1, no noise, with any field overridden (scalars or sequences by name)."""
    d = observe_desc_struct()
    load_library().qrgpu_observe_desc_default(C.byref(d), {"sim": OBS_SIM, "hardware": OBS_HARDWARE}[variant] if isinstance(variant, str) else int(variant))
    return _set_fields(d, fields)


JOY_ROWS, CMD_STATE_ROWS = 8, 6
RC_HARD_CODE, RC_JOY_TROT, RC_JOY_ADVANCED_TROT, RC_JOY_WALK, RC_JOY_STAND, RC_BODY_UP, RC_BODY_DOWN, RC_EXIT = range(8)


class command_desc_struct(C.Structure):
    _fields_ = [("dt", C.c_float), ("filter_factor", C.c_float), ("body_height", C.c_float), ("min_velx", C.c_float), ("max_velx", C.c_float),
                ("min_vely", C.c_float), ("max_vely", C.c_float), ("min_yawrate", C.c_float), ("max_yawrate", C.c_float), ("min_pitch", C.c_float),
                ("max_pitch", C.c_float)]


def command_desc(**fields):
    """qrgpu_command_desc: qrDesiredStateCommand's constants (dt 0.002, filter factor 0.02, body height 0.28, the velocity, yaw-rate and pitch
    clips), with any field overridden."""
    d = command_desc_struct()
    load_library().qrgpu_command_desc_default(C.byref(d))
    return _set_fields(d, fields)


class mpc_command_desc_struct(C.Structure):
    _fields_ = [("kp", C.c_float * 12), ("kd", C.c_float * 12), ("stance_kd", C.c_float), ("early_contact_abad_kp", C.c_float), ("epilogue", C.c_int)]


def mpc_command_desc(**fields):
    """qrgpu_mpc_command_desc: a1_sim's motor gains (100 / 1, 2, 2), stance Kd 3.0, EARLY_CONTACT abad Kp 100.0, epilogue 0 (the EPILOGUE_* bits the
    caller gave set_torque_epilogue), with any field overridden (scalars or sequences by name)."""
    d = mpc_command_desc_struct()
    load_library().qrgpu_mpc_command_desc_default(C.byref(d))
    return _set_fields(d, fields)


JOY_MSG_ROWS, FSM_SCRIPT_ROWS, FSM_SCRIPT_MAX, FSM_STATE_ROWS, FSM_OUT_ROWS = 10, 5, 64, 106, 11
FSM_ENTERED = 0x00010000                # in fsm_update's stage_mask: outside EP_REASONS and EP_BAD_FIELD
JOY_BTN_A, JOY_BTN_B, JOY_BTN_X, JOY_BTN_Y, JOY_BTN_RB, JOY_GAIT_SWITCH = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
FSM_PLAN_RUN, FSM_PLAN_PHASE1, FSM_PLAN_PHASE2, FSM_PLAN_ACTION, FSM_PLAN_HOLD, FSM_PLAN_PASSIVE, FSM_PLAN_REPEAT = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40
FSM_PLAN_DONE, FSM_PLAN_ACTION_FIRST, FSM_PLAN_ACTION_END = 0x100, 0x200, 0x400
FSM_PASSIVE, FSM_STAND_UP, FSM_LOCOMOTION = 1, 4, 7                       # FSM_StateName, row 0 of fsm_out
FSM_GAIT_TROT, FSM_GAIT_ADVANCED_TROT, FSM_GAIT_WALK, FSM_GAIT_STAND = 1, 2, 3, 4


class fsm_desc_struct(C.Structure):
    _fields_ = [("stand_up_angles", C.c_float * 12), ("sit_down_angles", C.c_float * 12), ("kp", C.c_float * 12), ("kd", C.c_float * 12),
                ("stand_up_time", C.c_float), ("stand_up_total", C.c_float), ("sit_down_time", C.c_float), ("time_step", C.c_float),
                ("transition_ticks", C.c_int), ("gait_transition_duration", C.c_float), ("stand_transition_duration", C.c_float),
                ("tau_clip", C.c_float), ("body_height", C.c_float), ("initial_ctrl_state", C.c_int), ("hard_code_v", C.c_float * 3),
                ("hard_code_w", C.c_float * 3), ("max_velx", C.c_float), ("max_vely", C.c_float), ("max_yawrate", C.c_float)]


def fsm_desc(**fields):
    """qrgpu_fsm_desc: the control state machine's constants -- a1_sim's stand-up and sit-down angles and motor gains, stand-up 2 s of 3 s, sit-down
    1.5 s, time step 0.001, transition_ticks 1000 with durations 2 (gait) and 1 (stand), torque clip 23, body height 0.28, constructed in BODY_UP --
    with any field overridden (scalars or sequences by name)."""
    d = fsm_desc_struct()
    load_library().qrgpu_fsm_desc_default(C.byref(d))
    return _set_fields(d, fields)


CHAIN_NONE, CHAIN_MPC, CHAIN_FORCE_BALANCE = 0, 1, 2    # qrgpu_mode_route_batch: the chain a robot is on
ROUTE_BAD_MODE, ROUTE_NO_CHAIN = 0x1, 0x2               # ... and the bits of route_flags


class mode_route_desc_struct(C.Structure):
    _fields_ = [("chain_of_mode", C.c_int * 4), ("fallback_chain", C.c_int)]


def mode_route_desc(**fields):
    """qrgpu_mode_route_desc: the chain of each LocomotionMode -- VELOCITY the force-balance chain, ADVANCED_TROT the MPC chain, POSITION and WALK none
    (such a robot runs on fallback_chain, the MPC chain, and is flagged) -- with any field overridden (scalars or sequences by name)."""
    d = mode_route_desc_struct()
    load_library().qrgpu_mode_route_desc_default(C.byref(d))
    return _set_fields(d, fields)


EPILOGUE_HIP_COMP, EPILOGUE_CLIP = 1, 2
COMM_ID_BYTES = 128


def comm_unique_id():
    """A fresh ncclUniqueId blob (rank 0 makes it; the launcher hands it to the other ranks)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = load_library().qrgpu_comm_unique_id(buf)
    if rc != 0:
        raise QrgpuError("qrgpu_comm_unique_id failed: %s" % ERRORS.get(rc, rc))
    return buf.raw


def lib_path():
    """The in-tree library; QRGPU_LIB names another build of it for A/B runs on one box (scratch/ab_bench.sh)."""
    return os.environ.get("QRGPU_LIB") or os.path.join(_HERE, "libqrgpu.so")


EXPORTS = ["qrgpu_model_desc_default", "qrgpu_create", "qrgpu_destroy", "qrgpu_set_stream", "qrgpu_get_stream", "qrgpu_last_error",
           "qrgpu_device_info", "qrgpu_mpc_setup", "qrgpu_wbc_setup", "qrgpu_mpc_solve_batch", "qrgpu_wbc_run_batch",
           "qrgpu_tick_batch", "qrgpu_mpc_solve1", "qrgpu_wbc_run1", "qrgpu_mpc_assemble_batch", "qrgpu_fb_debug_batch",
           "qrgpu_sync", "qrgpu_enable_timing", "qrgpu_get_timing", "qrgpu_malloc", "qrgpu_free", "qrgpu_memcpy_h2d",
           "qrgpu_memcpy_d2h", "qrgpu_mpc_frontend_batch", "qrgpu_set_lpt_schedule", "qrgpu_vmc_desc_default", "qrgpu_vmc_setup", "qrgpu_vmc_force_batch", "qrgpu_vmc_force1", "qrgpu_set_rescue_pass", "qrgpu_estimator_desc_default", "qrgpu_estimator_state_doubles",
           "qrgpu_estimator_update_batch", "qrgpu_pack_state_batch", "qrgpu_swing_targets_batch", "qrgpu_swing_velocity_batch", "qrgpu_gait_desc_default", "qrgpu_gait_update_batch",
           "qrgpu_foothold_desc_default", "qrgpu_footholds_batch", "qrgpu_ground_update_batch", "qrgpu_walk_gait_desc_default", "qrgpu_walk_gait_update_batch", "qrgpu_vmc_force_world_batch", "qrgpu_vmc_force_world1",
           "qrgpu_set_torque_epilogue", "qrgpu_comm_unique_id", "qrgpu_comm_init_rank", "qrgpu_comm_info", "qrgpu_comm_destroy",
           "qrgpu_allgather_tau", "qrgpu_allgather_tau_of_tick", "qrgpu_allgather_fence", "qrgpu_allgather_wait", "qrgpu_comm_sync", "qrgpu_set_warm_start", "qrgpu_set_planned_list",
           "qrgpu_enable_flop_count", "qrgpu_mpc_flop_counts", "qrgpu_mpc_set_hessian_mode", "qrgpu_wbc_inspect_batch", "qrgpu_host_alloc", "qrgpu_host_free",
           "qrgpu_memcpy_async", "qrgpu_memset_async", "qrgpu_mark", "qrgpu_mark_elapsed_ms", "qrgpu_set_tick_pipeline", "qrgpu_set_tick_overlap",
           "qrgpu_tick_fence", "qrgpu_tick_overlap_stats", "qrgpu_swing_mode_desc_default", "qrgpu_swing_update_batch", "qrgpu_swing_action_batch",
           "qrgpu_stance_desc_default", "qrgpu_stance_update_batch", "qrgpu_stance_command_batch", "qrgpu_stance_tick_batch",
           "qrgpu_pose_plan_desc_default", "qrgpu_pose_plan_batch", "qrgpu_plant_params_default", "qrgpu_forward_dynamics_batch", "qrgpu_plant_step_batch",
           "qrgpu_plant_step_terrain_batch", "qrgpu_plant_body_desc_default", "qrgpu_plant_body_setup", "qrgpu_plant_step_body_batch",
           "qrgpu_episode_desc_default", "qrgpu_episode_step_batch", "qrgpu_set_stage_reset",
           "qrgpu_observe_desc_default", "qrgpu_observe_state_rows", "qrgpu_observe_batch",
           "qrgpu_command_desc_default", "qrgpu_command_update_batch", "qrgpu_trot_inputs_batch", "qrgpu_mpc_command_desc_default",
           "qrgpu_mpc_command_batch", "qrgpu_tick_cadence_batch",
           "qrgpu_fsm_desc_default", "qrgpu_fsm_update_batch", "qrgpu_fsm_zero_command_batch", "qrgpu_fsm_command_batch",
           "qrgpu_gait_table_default", "qrgpu_gait_select_update_batch", "qrgpu_stage_clock_batch", "qrgpu_velocity_inputs_batch",
           "qrgpu_mode_route_desc_default", "qrgpu_mode_route_batch", "qrgpu_set_mode_route", "qrgpu_mode_command_batch"]


def load_library():
    """dlopen libqrgpu.so; raises MissingExtension when it was never built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # a context owns more streams than the HIP runtime's default of four hardware queues; streams that share a queue serialise each other and
    # the overlapped tick is refused (qrgpu_set_tick_overlap).  Read by the runtime at its first call in the process: a caller's own value stands.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    p = lib_path()
    if not os.path.exists(p):
        raise MissingExtension("%s not found: the HIP extension must be built first (no CPU fallback exists)" % p)
    lib = C.CDLL(p)
    vp, ip, fp = C.c_void_p, C.c_int, C.POINTER(C.c_float)
    lib.qrgpu_create.argtypes = [ip, ip, ip, C.POINTER(vp)]
    lib.qrgpu_destroy.argtypes = [vp]; lib.qrgpu_destroy.restype = None
    lib.qrgpu_set_stream.argtypes = [vp, vp]
    lib.qrgpu_get_stream.argtypes = [vp]
    lib.qrgpu_get_stream.restype = vp
    lib.qrgpu_set_lpt_schedule.argtypes = [vp, ip]
    lib.qrgpu_set_rescue_pass.argtypes = [vp, ip]
    lib.qrgpu_set_warm_start.argtypes = [vp, ip]
    lib.qrgpu_set_planned_list.argtypes = [vp, ip, ip]
    lib.qrgpu_enable_flop_count.argtypes = [vp, ip]
    lib.qrgpu_mpc_set_hessian_mode.argtypes = [vp, ip]
    lib.qrgpu_mpc_flop_counts.argtypes = [vp, C.POINTER(C.c_double)]
    lib.qrgpu_last_error.argtypes = [vp]; lib.qrgpu_last_error.restype = C.c_char_p
    lib.qrgpu_device_info.argtypes = [vp, C.c_char_p, ip, C.POINTER(ip)]
    lib.qrgpu_model_desc_default.argtypes = [C.POINTER(model_desc_struct)]; lib.qrgpu_model_desc_default.restype = None
    lib.qrgpu_mpc_setup.argtypes = [vp, ip, C.c_float, ip, C.c_float, C.c_float, C.c_float, fp, fp, C.c_float]
    lib.qrgpu_wbc_setup.argtypes = [vp, ip, C.POINTER(model_desc_struct)]
    lib.qrgpu_mpc_solve_batch.argtypes = [vp, ip] + [vp] * 8
    lib.qrgpu_wbc_run_batch.argtypes = [vp, ip] + [vp] * 7
    lib.qrgpu_wbc_inspect_batch.argtypes = [vp, ip] + [vp] * 7
    lib.qrgpu_tick_batch.argtypes = [vp, ip] + [vp] * 11
    if hasattr(lib, "qrgpu_tick_cadence_batch"):           # (an older build named by QRGPU_LIB for an A/B run has no cadenced tick)
        lib.qrgpu_tick_cadence_batch.argtypes = [vp, ip] + [vp] * 13
    lib.qrgpu_set_tick_overlap.argtypes = [vp, ip]
    lib.qrgpu_tick_fence.argtypes = [vp]
    lib.qrgpu_tick_overlap_stats.argtypes = [vp, C.POINTER(ip), C.POINTER(ip)]
    lib.qrgpu_set_torque_epilogue.argtypes = [vp, ip]
    lib.qrgpu_comm_unique_id.argtypes = [C.c_char_p]
    lib.qrgpu_comm_init_rank.argtypes = [vp, C.c_char_p, ip, ip]
    lib.qrgpu_comm_info.argtypes = [vp, C.POINTER(ip), C.POINTER(ip)]
    lib.qrgpu_comm_destroy.argtypes = [vp]
    lib.qrgpu_allgather_tau.argtypes = [vp, vp, vp, ip, vp, ip]
    lib.qrgpu_allgather_tau_of_tick.argtypes = [vp, vp, vp, ip, vp, ip]
    lib.qrgpu_allgather_fence.argtypes = [vp, ip]
    lib.qrgpu_allgather_wait.argtypes = [vp, ip]
    lib.qrgpu_comm_sync.argtypes = [vp]
    lib.qrgpu_mpc_assemble_batch.argtypes = [vp, ip] + [vp] * 6
    lib.qrgpu_vmc_desc_default.argtypes = [C.POINTER(vmc_desc_struct)]; lib.qrgpu_vmc_desc_default.restype = None
    lib.qrgpu_vmc_setup.argtypes = [vp, ip, C.POINTER(vmc_desc_struct)]
    lib.qrgpu_vmc_force_batch.argtypes = [vp, ip] + [vp] * 6
    lib.qrgpu_vmc_force_world_batch.argtypes = [vp, ip] + [vp] * 7
    lib.qrgpu_estimator_desc_default.argtypes = [C.POINTER(estimator_desc_struct)]; lib.qrgpu_estimator_desc_default.restype = None
    lib.qrgpu_estimator_state_doubles.argtypes = [ip]
    lib.qrgpu_estimator_update_batch.argtypes = [vp, ip, C.POINTER(estimator_desc_struct), vp, vp, vp, vp]
    lib.qrgpu_gait_desc_default.argtypes = [C.POINTER(gait_desc_struct)]; lib.qrgpu_gait_desc_default.restype = None
    lib.qrgpu_gait_update_batch.argtypes = [vp, ip, C.POINTER(gait_desc_struct), C.c_float, ip, ip, vp, vp, vp, vp]
    lib.qrgpu_walk_gait_desc_default.argtypes = [C.POINTER(walk_gait_desc_struct)]; lib.qrgpu_walk_gait_desc_default.restype = None
    lib.qrgpu_walk_gait_update_batch.argtypes = [vp, ip, C.POINTER(walk_gait_desc_struct), C.c_float, ip, ip, vp, vp, vp, vp, vp]
    lib.qrgpu_ground_update_batch.argtypes = [vp, ip, ip, vp, vp, vp, vp]
    lib.qrgpu_swing_velocity_batch.argtypes = [vp, ip, C.POINTER(estimator_desc_struct), C.POINTER(swing_velocity_desc_struct), vp, vp]
    lib.qrgpu_swing_targets_batch.argtypes = [vp, ip, C.POINTER(estimator_desc_struct), vp, vp, vp, vp]
    lib.qrgpu_foothold_desc_default.argtypes = [C.POINTER(foothold_desc_struct)]; lib.qrgpu_foothold_desc_default.restype = None
    lib.qrgpu_footholds_batch.argtypes = [vp, ip, C.POINTER(foothold_desc_struct), vp, vp, vp, vp]
    lib.qrgpu_pack_state_batch.argtypes = [vp, ip, fp, vp, vp, vp, vp, vp]
    lib.qrgpu_swing_mode_desc_default.argtypes = [C.POINTER(swing_mode_desc_struct), ip]; lib.qrgpu_swing_mode_desc_default.restype = None
    lib.qrgpu_swing_update_batch.argtypes = [vp, ip, C.POINTER(swing_mode_desc_struct), ip, ip] + [vp] * 9
    lib.qrgpu_swing_action_batch.argtypes = [vp, ip, C.POINTER(swing_mode_desc_struct), C.POINTER(estimator_desc_struct), ip] + [vp] * 7
    lib.qrgpu_stance_desc_default.argtypes = [C.POINTER(stance_desc_struct), ip]; lib.qrgpu_stance_desc_default.restype = None
    lib.qrgpu_stance_update_batch.argtypes = [vp, ip, C.POINTER(stance_desc_struct), C.c_float, ip, ip] + [vp] * 11
    lib.qrgpu_stance_command_batch.argtypes = [vp, ip, C.POINTER(stance_desc_struct), ip] + [vp] * 6
    lib.qrgpu_stance_tick_batch.argtypes = [vp, ip, C.POINTER(stance_desc_struct), C.c_float, ip, ip] + [vp] * 18
    lib.qrgpu_pose_plan_desc_default.argtypes = [C.POINTER(pose_plan_desc_struct)]; lib.qrgpu_pose_plan_desc_default.restype = None
    lib.qrgpu_pose_plan_batch.argtypes = [vp, ip, C.POINTER(pose_plan_desc_struct), ip, vp, ip] + [vp] * 9
    lib.qrgpu_plant_params_default.argtypes = [C.POINTER(plant_params_struct)]; lib.qrgpu_plant_params_default.restype = None
    lib.qrgpu_forward_dynamics_batch.argtypes = [vp, ip] + [vp] * 6
    lib.qrgpu_plant_step_batch.argtypes = [vp, ip, C.POINTER(plant_params_struct)] + [vp] * 7
    lib.qrgpu_plant_step_terrain_batch.argtypes = [vp, ip, C.POINTER(plant_params_struct), C.POINTER(terrain_desc_struct)] + [vp] * 11
    lib.qrgpu_plant_body_desc_default.argtypes = [C.POINTER(plant_body_desc_struct)]; lib.qrgpu_plant_body_desc_default.restype = None
    lib.qrgpu_plant_body_setup.argtypes = [vp, ip, C.POINTER(plant_body_desc_struct)]
    lib.qrgpu_plant_step_body_batch.argtypes = [vp, ip, C.POINTER(plant_params_struct), C.POINTER(terrain_desc_struct)] + [vp] * 12
    lib.qrgpu_episode_desc_default.argtypes = [C.POINTER(episode_desc_struct)]; lib.qrgpu_episode_desc_default.restype = None
    lib.qrgpu_episode_step_batch.argtypes = [vp, ip, C.POINTER(episode_desc_struct), ip, C.POINTER(plant_params_struct), C.POINTER(terrain_desc_struct), vp, vp, vp, ip] + [vp] * 11
    lib.qrgpu_set_stage_reset.argtypes = [vp, C.POINTER(stage_reset_struct)]
    lib.qrgpu_observe_desc_default.argtypes = [C.POINTER(observe_desc_struct), ip]; lib.qrgpu_observe_desc_default.restype = None
    lib.qrgpu_observe_state_rows.argtypes = [C.POINTER(observe_desc_struct)]
    lib.qrgpu_observe_batch.argtypes = [vp, ip, C.POINTER(observe_desc_struct), ip, C.c_uint] + [vp] * 7
    lib.qrgpu_command_desc_default.argtypes = [C.POINTER(command_desc_struct)]; lib.qrgpu_command_desc_default.restype = None
    lib.qrgpu_command_update_batch.argtypes = [vp, ip, C.POINTER(command_desc_struct), ip] + [vp] * 7
    lib.qrgpu_trot_inputs_batch.argtypes = [vp, ip] + [vp] * 9
    lib.qrgpu_mpc_command_desc_default.argtypes = [C.POINTER(mpc_command_desc_struct)]; lib.qrgpu_mpc_command_desc_default.restype = None
    lib.qrgpu_mpc_command_batch.argtypes = [vp, ip, C.POINTER(mpc_command_desc_struct), ip] + [vp] * 7
    lib.qrgpu_fsm_desc_default.argtypes = [C.POINTER(fsm_desc_struct)]; lib.qrgpu_fsm_desc_default.restype = None
    lib.qrgpu_fsm_update_batch.argtypes = [vp, ip, C.POINTER(fsm_desc_struct), ip, vp, vp, ip, vp, vp, C.c_uint] + [vp] * 4
    lib.qrgpu_fsm_zero_command_batch.argtypes = [vp, ip] + [vp] * 6
    lib.qrgpu_fsm_command_batch.argtypes = [vp, ip, C.POINTER(fsm_desc_struct)] + [vp] * 6
    lib.qrgpu_gait_table_default.argtypes = [C.POINTER(gait_desc_struct)]; lib.qrgpu_gait_table_default.restype = None
    lib.qrgpu_gait_select_update_batch.argtypes = [vp, ip, C.POINTER(gait_desc_struct), ip, vp, C.c_float, ip, ip] + [vp] * 6
    lib.qrgpu_stage_clock_batch.argtypes = [vp, ip, vp, C.c_uint, vp, vp, vp]
    if hasattr(lib, "qrgpu_velocity_inputs_batch"):        # (an older build named by QRGPU_LIB for an A/B run has no force-balance trot chain)
        lib.qrgpu_velocity_inputs_batch.argtypes = [vp, ip, ip, ip] + [vp] * 10
    if hasattr(lib, "qrgpu_mode_route_batch"):             # (... and none before the mode per robot knows these)
        lib.qrgpu_mode_route_desc_default.argtypes = [C.POINTER(mode_route_desc_struct)]; lib.qrgpu_mode_route_desc_default.restype = None
        lib.qrgpu_mode_route_batch.argtypes = [vp, ip, C.POINTER(mode_route_desc_struct)] + [vp] * 5
        lib.qrgpu_set_mode_route.argtypes = [vp, vp]
        lib.qrgpu_mode_command_batch.argtypes = [vp, ip] + [vp] * 7
    lib.qrgpu_vmc_force1.argtypes = [vp, ip, fp, fp, fp, fp, C.POINTER(ip)]
    lib.qrgpu_vmc_force_world1.argtypes = [vp, ip, fp, fp, fp, fp, fp, C.POINTER(ip)]
    lib.qrgpu_mpc_frontend_batch.argtypes = [vp, ip, ip, C.c_float, C.c_float] + [vp] * 6
    lib.qrgpu_fb_debug_batch.argtypes = [vp, ip, vp, vp, vp]
    lib.qrgpu_mpc_solve1.argtypes = [vp, ip] + [fp] * 9 + [C.POINTER(C.c_double), fp, C.POINTER(ip)]
    lib.qrgpu_wbc_run1.argtypes = [vp, ip] + [fp] * 6 + [C.POINTER(ip)]
    lib.qrgpu_sync.argtypes = [vp]
    lib.qrgpu_enable_timing.argtypes = [vp, ip]
    lib.qrgpu_get_timing.argtypes = [vp, ip, C.POINTER(C.c_double), C.POINTER(ip)]
    lib.qrgpu_malloc.argtypes = [vp, C.c_ulonglong]; lib.qrgpu_malloc.restype = vp
    lib.qrgpu_free.argtypes = [vp, vp]; lib.qrgpu_free.restype = None
    lib.qrgpu_memcpy_h2d.argtypes = [vp, vp, vp, C.c_ulonglong]
    lib.qrgpu_memcpy_d2h.argtypes = [vp, vp, vp, C.c_ulonglong]
    lib.qrgpu_host_alloc.restype = vp
    lib.qrgpu_host_alloc.argtypes = [vp, C.c_ulonglong]
    lib.qrgpu_host_free.argtypes = [vp, vp]
    lib.qrgpu_memcpy_async.argtypes = [vp, vp, vp, C.c_ulonglong, ip]
    lib.qrgpu_memset_async.argtypes = [vp, vp, ip, C.c_ulonglong]
    lib.qrgpu_mark.argtypes = [vp, ip]
    lib.qrgpu_mark_elapsed_ms.argtypes = [vp, ip, ip, C.POINTER(C.c_double)]
    _LIB = lib
    return lib


def _fill_gait_desc(d, cfg19):
    for l in range(4):
        d.stance_duration[l] = float(cfg19[l]); d.duty_factor[l] = float(cfg19[4 + l]); d.initial_leg_phase[l] = float(cfg19[8 + l])
        d.initial_leg_state[l] = int(cfg19[12 + l])
    d.contact_detection_phase_threshold = float(cfg19[16]); d.wait_time = float(cfg19[17]); d.advanced_trot = int(cfg19[18])


def gait_table_default():
    """qrgpu_gait_table_default: the five entries the FSM_GAIT_* values index ([0] the gait the generator is constructed with, trot, advanced_trot,
    walk, stand) as [5][19] float32 rows in workload.gait_cfg()'s layout."""
    d = (gait_desc_struct * 5)()
    load_library().qrgpu_gait_table_default(d)
    return np.array([[*e.stance_duration, *e.duty_factor, *e.initial_leg_phase, *e.initial_leg_state, e.contact_detection_phase_threshold, e.wait_time,
                      e.advanced_trot] for e in d], np.float32)


def _dp(x):
    """device pointer from an int, None, or an object with data_ptr()."""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class DeviceArray:
    """Minimal hipMalloc-backed array for callers that do not use torch (tests, smoke)."""

    def __init__(self, ctx, shape, dtype=np.float32):
        self.ctx, self.shape, self.dtype = ctx, tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.ptr = ctx._lib.qrgpu_malloc(ctx._h, max(self.nbytes, 8))
        if not self.ptr:
            raise QrgpuError("hipMalloc of %d bytes failed" % self.nbytes)

    def data_ptr(self):
        return self.ptr

    def upload(self, host):
        host = np.ascontiguousarray(host, self.dtype)
        assert host.nbytes == self.nbytes, (host.shape, self.shape)
        self.ctx._chk(self.ctx._lib.qrgpu_memcpy_h2d(self.ctx._h, self.ptr, host.ctypes.data, self.nbytes))
        return self

    def download(self):
        out = np.empty(self.shape, self.dtype)
        self.ctx._chk(self.ctx._lib.qrgpu_memcpy_d2h(self.ctx._h, out.ctypes.data, self.ptr, self.nbytes))
        return out

    def zero(self):
        """Asynchronous byte fill with 0 on the context stream."""
        self.ctx._chk(self.ctx._lib.qrgpu_memset_async(self.ctx._h, self.ptr, 0, self.nbytes))
        return self

    def copy_from_pinned(self, pinned):
        """Asynchronous host -> device copy from a PinnedArray of the same size."""
        assert pinned.nbytes == self.nbytes
        self.ctx._chk(self.ctx._lib.qrgpu_memcpy_async(self.ctx._h, self.ptr, pinned.ptr, self.nbytes, 0))
        return self

    def copy_to_pinned(self, pinned):
        assert pinned.nbytes == self.nbytes
        self.ctx._chk(self.ctx._lib.qrgpu_memcpy_async(self.ctx._h, pinned.ptr, self.ptr, self.nbytes, 1))
        return pinned

    def row(self, r0, r1=None):
        """Device pointer (int) of rows [r0, r1) of a 2-d array, e.g. the joint angles inside fb_state."""
        return self.ptr + r0 * int(np.prod(self.shape[1:])) * self.dtype.itemsize

    def free(self):
        if self.ptr:
            self.ctx._lib.qrgpu_free(self.ctx._h, self.ptr)
            self.ptr = None


class PinnedArray:
    """hipHostMalloc-backed numpy view (qrgpu_host_alloc) for asynchronous copies."""

    def __init__(self, ctx, shape, dtype=np.float32):
        self.ctx, self.shape, self.dtype = ctx, tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.ptr = ctx._lib.qrgpu_host_alloc(ctx._h, max(self.nbytes, 8))
        if not self.ptr:
            raise QrgpuError("hipHostMalloc of %d bytes failed" % self.nbytes)
        self.array = np.ctypeslib.as_array((C.c_char * self.nbytes).from_address(self.ptr)).view(self.dtype).reshape(self.shape)

    def free(self):
        if self.ptr:
            self.array = None
            self.ctx._lib.qrgpu_host_free(self.ctx._h, self.ptr)
            self.ptr = None


class Context:
    """One qrgpu_ctx: a device, a stream, per-type MPC/WBC parameters."""

    def __init__(self, device_id=0, max_batch=1024, horizon_max=16):
        self._lib = load_library()
        h = C.c_void_p()
        rc = self._lib.qrgpu_create(device_id, max_batch, horizon_max, C.byref(h))
        if rc != 0:
            raise QrgpuError("qrgpu_create failed: %s (a gfx950 device is required; there is no CPU fallback)" % ERRORS.get(rc, rc))
        self._h = h
        self.max_batch, self.horizon = max_batch, None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.qrgpu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise QrgpuError("%s: %s" % (ERRORS.get(rc, rc), self._lib.qrgpu_last_error(self._h).decode()))

    def last_error(self):
        return self._lib.qrgpu_last_error(self._h).decode()

    # -- setup ---------------------------------------------------------------------------------
    def set_stream(self, stream_ptr):
        self._chk(self._lib.qrgpu_set_stream(self._h, C.c_void_p(int(stream_ptr) if stream_ptr else 0)))

    def get_stream(self):
        """The hipStream_t (as an integer) the context queues on: a non-blocking stream of its own unless set_stream named another."""
        return int(self._lib.qrgpu_get_stream(self._h) or 0)

    def device_info(self):
        buf = C.create_string_buffer(256); lds = C.c_int(0)
        cus = self._lib.qrgpu_device_info(self._h, buf, 256, C.byref(lds))
        return dict(name=buf.value.decode(), cus=cus, lds_per_cu=lds.value)

    def mpc_setup(self, type_id, dt, horizon, mu, fmax, mass, inertia, weights, alpha):
        inertia = np.ascontiguousarray(inertia, np.float32); weights = np.ascontiguousarray(weights, np.float32)
        self._chk(self._lib.qrgpu_mpc_setup(self._h, type_id, dt, horizon, mu, fmax, mass, _fp(inertia), _fp(weights), alpha))
        self.horizon = horizon

    def mpc_setup_packed(self, type_id, cfg20, horizon):
        """cfg20 = dt, mu, fmax, mass, inertia[3], weights[12], alpha (workload.mpc_cfg)."""
        c = np.asarray(cfg20, np.float32)
        self.mpc_setup(type_id, float(c[0]), horizon, float(c[1]), float(c[2]), float(c[3]), c[4:7], c[7:19], float(c[19]))

    def wbc_setup(self, type_id, hip_l=None, upper_l=None, lower_l=None, body_size=None, **gains):
        d = model_desc_struct()
        self._lib.qrgpu_model_desc_default(C.byref(d))
        _set_fields(d, dict(hip_l=hip_l, upper_l=upper_l, lower_l=lower_l, body_size=None if body_size is None else [body_size[i] for i in range(3)], **gains))
        self._chk(self._lib.qrgpu_wbc_setup(self._h, type_id, C.byref(d)))

    def wbc_setup_packed(self, type_id, model6):
        m = np.asarray(model6, np.float32)
        self.wbc_setup(type_id, float(m[0]), float(m[1]), float(m[2]), [float(x) for x in m[3:6]])

    def alloc(self, shape, dtype=np.float32):
        return DeviceArray(self, shape, dtype)

    def alloc_pinned(self, shape, dtype=np.float32):
        return PinnedArray(self, shape, dtype)

    def copy_rows(self, dst, src, count, dtype=np.float32):
        """Asynchronous device -> device copy of `count` elements on the context stream (dst, src: device pointers, e.g. DeviceArray.row())."""
        self._chk(self._lib.qrgpu_memcpy_async(self._h, _dp(dst), _dp(src), int(count) * np.dtype(dtype).itemsize, 2))

    def mark(self, index):
        """Record timing mark `index` on the context stream."""
        self._chk(self._lib.qrgpu_mark(self._h, int(index)))

    def mark_elapsed_ms(self, a, b):
        ms = C.c_double(0)
        self._chk(self._lib.qrgpu_mark_elapsed_ms(self._h, int(a), int(b), C.byref(ms)))
        return ms.value

    # -- batched device-pointer API ---------------------------------------------------------------
    def mpc_solve_batch(self, n, mpc_state, traj, gait, q, force, tau=None, status=None, type_id=None):
        self._chk(self._lib.qrgpu_mpc_solve_batch(self._h, n, _dp(type_id), _dp(mpc_state), _dp(traj), _dp(gait), _dp(q),
                                                  _dp(force), _dp(tau), _dp(status)))

    def wbc_run_batch(self, n, fb_state, wbc_cmd, prev_ori, tau, qdes=None, status=None, type_id=None):
        self._chk(self._lib.qrgpu_wbc_run_batch(self._h, n, _dp(type_id), _dp(fb_state), _dp(wbc_cmd), _dp(prev_ori), _dp(tau),
                                                _dp(qdes), _dp(status)))

    def wbc_inspect_batch(self, n, fb_state, wbc_cmd, prev_ori, tau, qp, status=None, type_id=None):
        """wbc_run_batch plus the relaxation QP's solution: qp [n][30] = qpz[18], optimalFr[12] (instrumented kernel)."""
        self._chk(self._lib.qrgpu_wbc_inspect_batch(self._h, n, _dp(type_id), _dp(fb_state), _dp(wbc_cmd), _dp(prev_ori), _dp(tau),
                                                    _dp(qp), _dp(status)))

    def tick_batch(self, n, mpc_state, traj, gait, fb_state, wbc_cmd, prev_ori, force, tau, status=None, type_id=None, qdes=None):
        """qdes [24][n]: desiredJPos / desiredJVel of the kinematic projection (K12); None skips that projection."""
        self._chk(self._lib.qrgpu_tick_batch(self._h, n, _dp(type_id), _dp(mpc_state), _dp(traj), _dp(gait), _dp(fb_state),
                                             _dp(wbc_cmd), _dp(prev_ori), _dp(force), _dp(tau), _dp(qdes), _dp(status)))

    def tick_cadence_batch(self, n, updated, mpc_state, traj, gait, fb_state, wbc_cmd, prev_ori, force, hold, tau, status=None, qdes=None, type_id=None):
        """The tick on the reference's cadence: robots whose word of `updated` [n] (int32, what mpc_frontend_batch writes) is non-zero are solved and
        command their MPC torques, the others command the held base-frame force through the current Jacobian and run the WBC.  force and hold
        [12][n] are memory carried from call to call (include/qrgpu.h).  Always the serial form on the context's stream."""
        self._chk(self._lib.qrgpu_tick_cadence_batch(self._h, n, _dp(type_id), _dp(updated), _dp(mpc_state), _dp(traj), _dp(gait), _dp(fb_state),
                                                     _dp(wbc_cmd), _dp(prev_ori), _dp(force), _dp(hold), _dp(tau), _dp(qdes), _dp(status)))

    def set_tick_pipeline(self, on=True):
        """WBC launch of a tick beside its MPC launches (default) or behind them."""
        self._chk(self._lib.qrgpu_set_tick_pipeline(self._h, 1 if on else 0))

    def set_tick_overlap(self, on=True, strict=True):
        """Consecutive pipelined ticks (h <= 11) that write different output arrays overlap: tick t + 1's solves start in tick t's drain
        (include/qrgpu.h: the caller's promise about inputs).  -> True when the mode is on.  The library refuses it when two of the context's
        streams share a hardware queue (GPU_MAX_HW_QUEUES): strict raises, otherwise False is returned and ticks stay as they were."""
        rc = self._lib.qrgpu_set_tick_overlap(self._h, 1 if on else 0)
        if rc == 3 and not strict:             # QRGPU_ERR_NOT_SETUP
            return False
        self._chk(rc)
        return bool(on)

    def tick_overlap_stats(self):
        """-> (ticks chained to their predecessor, overlapped-form ticks that waited for the context's stream instead)"""
        a, b = C.c_int(0), C.c_int(0)
        self._chk(self._lib.qrgpu_tick_overlap_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def tick_fence(self):
        """The next overlapped tick waits for everything queued on the context's stream so far (inputs produced there since the last tick)."""
        self._chk(self._lib.qrgpu_tick_fence(self._h))

    def set_torque_epilogue(self, hip_comp=False, clip=False):
        """K14 tail on the batched torques: +-0.9 N m abad compensation (qr_fsm_state_locomotion.cpp:141-151), +-23 N m clip (qr_safety_checker.cpp:48-66)."""
        self._chk(self._lib.qrgpu_set_torque_epilogue(self._h, (EPILOGUE_HIP_COMP if hip_comp else 0) | (EPILOGUE_CLIP if clip else 0)))

    def vmc_setup_packed(self, type_id, cfg20, geom3):
        """cfg20 = workload.vmc_cfg(): mass, inertia[9], acc_weight[6], reg_weight, friction, fmin_ratio, fmax_ratio; geom3 = hip/upper/lower length."""
        d = vmc_desc_struct()
        cfg20 = np.asarray(cfg20, np.float32)
        d.mass = float(cfg20[0])
        for i in range(9): d.inertia[i] = float(cfg20[1 + i])
        for i in range(6): d.acc_weight[i] = float(cfg20[10 + i])
        d.reg_weight, d.friction, d.fmin_ratio, d.fmax_ratio = (float(v) for v in cfg20[16:20])
        d.hip_l, d.upper_l, d.lower_l = (float(v) for v in geom3[:3])
        self._chk(self._lib.qrgpu_vmc_setup(self._h, type_id, C.byref(d)))

    def vmc_force_batch(self, n, vmc_in, q, force, tau=None, status=None, type_id=None):
        """ComputeContactForce (+ MapContactForceToJointTorques) of n robots: qr_qp_torque_optimizer.cpp:190-301."""
        self._chk(self._lib.qrgpu_vmc_force_batch(self._h, n, _dp(type_id), _dp(vmc_in), _dp(q), _dp(force), _dp(tau), _dp(status)))

    def vmc_force_world_batch(self, n, vmc_in, ratio, q, force, tau=None, status=None, type_id=None):
        """World-frame overload (qr_qp_torque_optimizer.cpp:304-398): vmc_in carries Rcb = rotMat, gvec = (0,0,9.8), normal = e_z; ratio [8][n]."""
        self._chk(self._lib.qrgpu_vmc_force_world_batch(self._h, n, _dp(type_id), _dp(vmc_in), _dp(ratio), _dp(q), _dp(force), _dp(tau), _dp(status)))

    def vmc_force1(self, vmc_in, q=None, type_id=0):
        a = np.ascontiguousarray(vmc_in, np.float32); qa = np.ascontiguousarray(q, np.float32) if q is not None else None
        f = np.zeros(12, np.float32); tau = np.zeros(12, np.float32); st = C.c_int(0)
        self._chk(self._lib.qrgpu_vmc_force1(self._h, type_id, _fp(a), _fp(qa) if qa is not None else None, _fp(f),
                                             _fp(tau) if qa is not None else None, C.byref(st)))
        return f, (tau if qa is not None else None), st.value

    def vmc_force_world1(self, vmc_in, ratio, q=None, type_id=0):
        """One robot through the world-frame overload (qrgpu_vmc_force_world1): ratio = fMinRatio[4], fMaxRatio[4]."""
        a = np.ascontiguousarray(vmc_in, np.float32); r = np.ascontiguousarray(ratio, np.float32)
        qa = np.ascontiguousarray(q, np.float32) if q is not None else None
        f = np.zeros(12, np.float32); tau = np.zeros(12, np.float32); st = C.c_int(0)
        self._chk(self._lib.qrgpu_vmc_force_world1(self._h, type_id, _fp(a), _fp(r), _fp(qa) if qa is not None else None, _fp(f),
                                                   _fp(tau) if qa is not None else None, C.byref(st)))
        return f, (tau if qa is not None else None), st.value

    def estimator_state_doubles(self, window):
        return self._lib.qrgpu_estimator_state_doubles(int(window))

    def estimator_update_batch(self, n, cfg20, est_in, tick, est_state, est_out):
        """UpdateDataFlow kinematics + qrRobotVelocityEstimator::Update of n robots.  cfg20 = workload.estimator_cfg()."""
        d = _estimator_desc(cfg20)
        self._chk(self._lib.qrgpu_estimator_update_batch(self._h, n, C.byref(d), _dp(est_in), _dp(tick), _dp(est_state), _dp(est_out)))

    def gait_update_batch(self, n, cfg19, current_time, contact, gait_state, gait_out=None, fe_in=None, stop=False, reset=False):
        """qrOpenLoopGaitGenerator::Update of n robots (qr_openloop_gait_generator.cpp:126-249).  cfg19 = workload.gait_cfg().
        reset: True / GAIT_RESET_CONSTRUCT (1) = start from a generator as constructed, GAIT_RESET_LIVE (2) = Reset(0) on the running generator --
        the other way round from walk_gait_update_batch / swing_update_batch (include/qrgpu.h); any other value is refused."""
        d = gait_desc_struct()
        _fill_gait_desc(d, np.asarray(cfg19, np.float32))
        self._chk(self._lib.qrgpu_gait_update_batch(self._h, n, C.byref(d), float(current_time), int(bool(stop)), int(reset), _dp(contact),
                                                    _dp(gait_state), _dp(gait_out), _dp(fe_in)))

    def gait_select_update_batch(self, n, table, sel, current_time, contact, gait_state, gait_out=None, fe_in=None, swing_in=None, flags=None, stop=False,
                                 reset=0):
        """gait_update_batch with the gait per robot: table = a list of the 19-float rows workload.gait_cfg() makes (workload.gait_table(): [5][19]; at
        most MAX_GAITS), sel [n] float32 on the device = each robot's index in it (row 44 of fsm_state: fsm_state.row(44)), read only where the robot
        is reset at this call -- reset (0, GAIT_RESET_CONSTRUCT, GAIT_RESET_LIVE) if non-zero, else the level of set_stage_reset where its mask says --
        and kept in row 48 of gait_state.  A bad selection runs entry 0 and sets GAIT_BAD_SEL in flags [n] int32.  swing_in: rows 8-11 receive the
        swingDuration of the gait in force."""
        key = np.asarray(table, np.float32).tobytes()
        if getattr(self, "_gait_table", (None,))[0] != key:             # a loop passes the same table every tick: its structs are made once
            rows = [np.asarray(r, np.float32) for r in table]
            d = (gait_desc_struct * max(len(rows), 1))()
            for e, r in zip(d, rows):
                _fill_gait_desc(e, r)
            self._gait_table = (key, d, len(rows))
        _, d, count = self._gait_table
        self._chk(self._lib.qrgpu_gait_select_update_batch(self._h, n, d, count, _dp(sel), float(current_time), int(bool(stop)), int(reset), _dp(contact),
                                                           _dp(gait_state), _dp(gait_out), _dp(fe_in), _dp(swing_in), _dp(flags)))

    def stage_clock(self, n, mask, bits, ticks, origin, local):
        """The stage clock that restarts where the mask says: origin[r] = ticks[r] where (mask[r] & bits) != 0, then local[r] = ticks[r] - origin[r]
        (all [n] int32 on the device; origin is the clock's memory: zeroed, or every robot masked at the first call).  With mask = fsm_update's
        stage_mask, bits = EP_REASONS | FSM_ENTERED, ticks = row 0 of ep_state and local given to set_stage_reset as its ticks, the stages' clock counts
        from the robot's last OnEnter or spawn."""
        self._chk(self._lib.qrgpu_stage_clock_batch(self._h, n, _dp(mask), int(bits), _dp(ticks), _dp(origin), _dp(local)))

    def walk_gait_update_batch(self, n, cfg26, current_time, contact, walk_state, walk_out=None, ratio=None, vmc_in=None, stop=False, reset=0):
        """qrWalkGaitGenerator::Update of n robots + the walk branch of UpdateFRatio (qr_walk_gait_generator.cpp:202-288,
        qr_torque_stance_leg_controller.cpp:125-168).  cfg26 = workload.walk_cfg(); reset: 2 = as constructed, 1 = Reset(), 0 = carry on."""
        d = walk_gait_desc_struct()
        v = np.asarray(cfg26, np.float32)
        for l in range(4):
            d.stance_duration[l] = float(v[l]); d.duty_factor[l] = float(v[4 + l]); d.initial_leg_phase[l] = float(v[8 + l]); d.initial_leg_state[l] = int(v[12 + l])
            d.state_switch[l] = int(v[18 + l]); d.state_ratio[l] = float(v[22 + l])
        d.contact_detection_phase_threshold = float(v[16]); d.n_states = int(v[17])
        self._chk(self._lib.qrgpu_walk_gait_update_batch(self._h, n, C.byref(d), float(current_time), int(bool(stop)), int(reset), _dp(contact),
                                                         _dp(walk_state), _dp(walk_out), _dp(ratio), _dp(vmc_in)))

    def ground_update_batch(self, n, ground_in, ground_state, ground_out=None, est_in=None, reset=False):
        """qrGroundSurfaceEstimator::Update of n robots (qr_ground_surface_estimator.cpp:40-70,151-206): ground_in [23][n],
        ground_state [13][n] doubles (memory), ground_out [32][n]; est_in: rows 45-53 receive groundRMat."""
        self._chk(self._lib.qrgpu_ground_update_batch(self._h, n, int(bool(reset)), _dp(ground_in), _dp(ground_state), _dp(ground_out), _dp(est_in)))

    def footholds_batch(self, n, desc29, fh_in, swing_in, gait_state=None, gait_out=None):
        """Swing-leg selection + foothold heuristic (qr_swing_leg_controller.cpp:211-236, qr_foothold_planner.cpp:110-239).
        desc29 = workload.foothold_cfg(): hip_offset[12], default_hip_position[12], hip_l, swing_kp[3], foot_clearance."""
        d = foothold_desc_struct()
        self._lib.qrgpu_foothold_desc_default(C.byref(d))
        v = np.asarray(desc29, np.float32)
        for i in range(12):
            d.hip_offset[i] = float(v[i]); d.default_hip_position[i] = float(v[12 + i])
        d.hip_l = float(v[24]); d.foot_clearance = float(v[28])
        for i in range(3):
            d.swing_kp[i] = float(v[25 + i])
        self._chk(self._lib.qrgpu_footholds_batch(self._h, n, C.byref(d), _dp(fh_in), _dp(gait_state), _dp(gait_out), _dp(swing_in)))

    def swing_velocity_batch(self, n, cfg20, vdesc20, swing_vel_in, out):
        """Swing-leg action of the velocity mode (qr_swing_leg_controller.cpp:285-309, 408-424).  cfg20 = workload.estimator_cfg() (geometry
        part), vdesc20 = workload.swing_velocity_cfg(): hip position + com offset[12], stanceDuration[4], swingKp[3], desiredHeight - clearance."""
        d = _estimator_desc(cfg20, geometry_only=True)
        v = swing_velocity_desc_struct(); vd = np.asarray(vdesc20, np.float32)
        for i in range(12): v.hip_position_com[i] = float(vd[i])
        for i in range(4): v.stance_duration[i] = float(vd[12 + i])
        for i in range(3): v.swing_kp[i] = float(vd[16 + i])
        v.desired_height = float(vd[19])
        self._chk(self._lib.qrgpu_swing_velocity_batch(self._h, n, C.byref(d), C.byref(v), _dp(swing_vel_in), _dp(out)))

    def swing_targets_batch(self, n, cfg20, swing_in, wbc_cmd=None, foot_target_world=None, qdes=None):
        """Swing-leg targets (qr_swing_leg_controller.cpp:362-424, ADVANCED_TROT).  cfg20 = workload.estimator_cfg() (geometry part)."""
        d = _estimator_desc(cfg20, geometry_only=True)
        self._chk(self._lib.qrgpu_swing_targets_batch(self._h, n, C.byref(d), _dp(swing_in), _dp(wbc_cmd), _dp(foot_target_world), _dp(qdes)))

    def swing_update_batch(self, n, desc, est_in, est_out, gait_out, swing_state, swing_flags, gait_state=None, swing_in=None, swing_vel_in=None,
                           fe_in=None, reset=0, stop=False):
        """qrRaibertSwingLegController::Reset (reset: 2 = constructed, 1 = Reset(), 0 = carry on) + Update of n robots: the lift-off memory
        of every mode, the footholds and walk trajectories (qr_swing_leg_controller.cpp:60-196).  desc = swing_mode_desc(mode, ...)."""
        self._chk(self._lib.qrgpu_swing_update_batch(self._h, n, C.byref(desc), int(reset), int(bool(stop)), _dp(est_in), _dp(est_out), _dp(gait_out),
                                                     _dp(gait_state), _dp(swing_state), _dp(swing_in), _dp(swing_vel_in), _dp(fe_in), _dp(swing_flags)))

    def swing_action_batch(self, n, desc, cfg20, est_in, est_out, gait_out, swing_state, out, swing_flags, gait_state=None, stop=False):
        """GetAction of the position and walk modes (qr_swing_leg_controller.cpp:204-229, 311-359, 407-459).  cfg20 = workload.estimator_cfg()
        (geometry part); out [52][n]."""
        d = _estimator_desc(cfg20, geometry_only=True)
        self._chk(self._lib.qrgpu_swing_action_batch(self._h, n, C.byref(desc), C.byref(d), int(bool(stop)), _dp(est_in), _dp(est_out), _dp(gait_out),
                                                     _dp(gait_state), _dp(swing_state), _dp(out), _dp(swing_flags)))

    def stance_update_batch(self, n, desc, est_in, est_out, ground_out, rpy, gait_out, stance_cmd, stance_state, gait_state=None, vmc_in=None,
                            ratio=None, stance_out=None, current_time=0.0, stop=False, reset=False):
        """TorqueStanceLegController::UpdateFRatio + UpdateDesCommand of n robots (qr_torque_stance_leg_controller.cpp:89-477): the complete
        vmc_in [37][n], ratio [8][n] and stance_out [33][n] from arrays the device holds.  desc = stance_desc(mode, ...)."""
        self._chk(self._lib.qrgpu_stance_update_batch(self._h, n, C.byref(desc), float(current_time), int(bool(stop)), int(bool(reset)), _dp(est_in),
                                                      _dp(est_out), _dp(ground_out), _dp(rpy), _dp(gait_out), _dp(gait_state), _dp(stance_cmd),
                                                      _dp(stance_state), _dp(vmc_in), _dp(ratio), _dp(stance_out)))

    def pose_plan_batch(self, n, desc, est_in, est_out, ground_out, rpy, walk_out, pose_state, stance_cmd, pose_flags, event=POSE_EVENT_SWITCH_TO_SWING,
                        event_words=None, pose_out=None, reset=False):
        """qrPosePlanner::Update (the 20-iteration SQP) / ResetBasePose of n robots (qr_pose_planner.cpp:72-456): rows 7-24 of stance_cmd
        [28][n] from arrays the device holds.  event: POSE_EVENT_*; event_words [n] int32 (0 / 1 / 2 per robot) wins when given.
        desc = pose_plan_desc(...); pose_state [26][n]; pose_flags [n] int32 of PP_* bits; pose_out [178][n] or None."""
        self._chk(self._lib.qrgpu_pose_plan_batch(self._h, n, C.byref(desc), int(event), _dp(event_words), int(bool(reset)), _dp(est_in), _dp(est_out),
                                                  _dp(ground_out), _dp(rpy), _dp(walk_out), _dp(pose_state), _dp(stance_cmd), _dp(pose_out),
                                                  _dp(pose_flags)))

    def stance_command_batch(self, n, desc, tau, motor_cmd, vmc_in=None, stance_out=None, swing_q=None, swing_flag=None, stop=False):
        """The motor-command tail of GetAction (:503-541) merged with the swing command (qr_locomotion_controller.cpp:128-147):
        motor_cmd [60][n] = p, Kp, d, Kd, tua.  vmc_in / stance_out: WALK only; swing_q [24][n], swing_flag [4][n]: both or neither."""
        self._chk(self._lib.qrgpu_stance_command_batch(self._h, n, C.byref(desc), int(bool(stop)), _dp(vmc_in), _dp(stance_out), _dp(tau), _dp(swing_q),
                                                       _dp(swing_flag), _dp(motor_cmd)))

    def stance_tick_batch(self, n, desc, est_in, est_out, ground_out, rpy, gait_out, stance_cmd, stance_state, vmc_in, force, tau, motor_cmd,
                          gait_state=None, ratio=None, stance_out=None, status=None, swing_q=None, swing_flag=None, type_id=None, current_time=0.0,
                          stop=False, reset=False):
        """stance_update_batch, the force-balance QP overload the mode selects, stance_command_batch: three launches on the context's stream."""
        self._chk(self._lib.qrgpu_stance_tick_batch(self._h, n, C.byref(desc), float(current_time), int(bool(stop)), int(bool(reset)), _dp(type_id),
                                                    _dp(est_in), _dp(est_out), _dp(ground_out), _dp(rpy), _dp(gait_out), _dp(gait_state), _dp(stance_cmd),
                                                    _dp(stance_state), _dp(vmc_in), _dp(ratio), _dp(stance_out), _dp(force), _dp(tau), _dp(status),
                                                    _dp(swing_q), _dp(swing_flag), _dp(motor_cmd)))

    def pack_state_batch(self, n, com_offset, est_in, est_out, rpy, mpc_state=None, fb_state=None):
        """mpc_state[28] / fb_state[37] from the estimator's inputs and outputs (SolveDenseMPC :385-399, UpdateModel :136-156)."""
        co = np.ascontiguousarray(com_offset, np.float32)
        self._chk(self._lib.qrgpu_pack_state_batch(self._h, n, _fp(co), _dp(est_in), _dp(est_out), _dp(rpy), _dp(mpc_state), _dp(fb_state)))

    def forward_dynamics_batch(self, n, fb_state, tau, nu_dot, foot_force=None, status=None, type_id=None):
        """nu_dot [18][n] = d/dt of (omega_body, v_body, qd) under tau [12][n] and the world-frame foot forces [12][n] (None: none):
        FloatingBaseModel::runABA with _externalForces, rotor terms included."""
        self._chk(self._lib.qrgpu_forward_dynamics_batch(self._h, n, _dp(type_id), _dp(fb_state), _dp(tau), _dp(foot_force), _dp(nu_dot), _dp(status)))

    def plant_step_batch(self, n, params, fb_state, motor_cmd, plant_out=None, mpc_state=None, est_in=None, status=None, type_id=None):
        """fb_state [37][n] advances in place by one control tick of the simulated robots (params: plant_params()): motor law on motor_cmd
        [60][n], ground contact, forward dynamics, semi-implicit Euler.  plant_out [PLANT_OUT_ROWS][n], the ground-truth mpc_state [28][n]
        and rows 0-40 of est_in [54][n] are written when given."""
        self._chk(self._lib.qrgpu_plant_step_batch(self._h, n, C.byref(params), _dp(type_id), _dp(fb_state), _dp(motor_cmd), _dp(plant_out),
                                                   _dp(mpc_state), _dp(est_in), _dp(status)))

    def plant_step_terrain_batch(self, n, params, terrain, height, fb_state, motor_cmd, field_id=None, base_push=None, plant_out=None, terrain_out=None,
                                 mpc_state=None, est_in=None, status=None, type_id=None):
        """plant_step_batch on a height field: terrain = terrain_desc(), height [n_fields][ny][nx] float32 on the device, field_id [n] int32
        (None: field 0), base_push [6][n] = world-frame force at the base origin and moment, held over the tick (None: none).  terrain_out
        [TERRAIN_OUT_ROWS][n]: ground height under each foot and the unit normal there, of the state written."""
        self._chk(self._lib.qrgpu_plant_step_terrain_batch(self._h, n, C.byref(params), C.byref(terrain), _dp(height), _dp(field_id), _dp(base_push),
                                                           _dp(type_id), _dp(fb_state), _dp(motor_cmd), _dp(plant_out), _dp(terrain_out), _dp(mpc_state),
                                                           _dp(est_in), _dp(status)))

    def plant_body_setup(self, type_id, desc):
        """The body of robot type type_id (plant_body_desc()): what plant_step_body_batch needs for every type set up with wbc_setup."""
        self._chk(self._lib.qrgpu_plant_body_setup(self._h, type_id, C.byref(desc)))

    def plant_step_body_batch(self, n, params, terrain, height, fb_state, motor_cmd, field_id=None, base_push=None, plant_out=None, terrain_out=None,
                              body_out=None, mpc_state=None, est_in=None, status=None, type_id=None):
        """plant_step_terrain_batch for robots with a body: the knees and the eight trunk corners touch the ground by the feet's law, the joints
        have stops.  body_out [BODY_OUT_ROWS][n]: knee force, knee contact, the corners' f_n, the stops' torques, of the last sub-step; status
        names a fall (PL_TRUNK_CONTACT, PL_KNEE_CONTACT) and a joint at a stop (PL_JOINT_LIMIT)."""
        self._chk(self._lib.qrgpu_plant_step_body_batch(self._h, n, C.byref(params), C.byref(terrain), _dp(height), _dp(field_id), _dp(base_push),
                                                        _dp(type_id), _dp(fb_state), _dp(motor_cmd), _dp(plant_out), _dp(terrain_out), _dp(body_out),
                                                        _dp(mpc_state), _dp(est_in), _dp(status)))

    def episode_step_batch(self, n, desc, fb_state, spawn, n_spawn, ep_state, ep_stats, done, reset_all=False, params=None, terrain=None, height=None,
                           field_id=None, plant_status=None, tick_status=None, force_reset=None, prev_ori=None, motor_cmd=None, done_list=None,
                           done_count=None):
        """Per-robot termination, reset and spawn (desc: episode_desc()): done [n] gets each robot's EP_* reason bits; a robot whose episode ends
        is spawned from the table spawn [4][n_spawn] (x, y, yaw, reserved) into fb_state [37][n], with prev_ori [3][n] zeroed and its motor_cmd
        [60][n] column set to a joint PD hold (both optional).  ep_state [EPISODE_STATE_ROWS][n] int32 and ep_stats [EPISODE_STATS_ROWS][n] carry
        the bookkeeping; reset_all starts every robot at episode 0 (the first call on new arrays).  terrain / height / field_id as in
        plant_step_terrain_batch (None: flat at params.ground_z; params None: 0).  done_list [n], done_count [1] int32: the robots reset, compacted,
        in no fixed order.  Intended loop: episode step, plant step, tick."""
        self._chk(self._lib.qrgpu_episode_step_batch(self._h, n, C.byref(desc), int(bool(reset_all)), None if params is None else C.byref(params),
                                                     None if terrain is None else C.byref(terrain), _dp(height), _dp(field_id), _dp(spawn), int(n_spawn),
                                                     _dp(plant_status), _dp(tick_status), _dp(force_reset), _dp(fb_state), _dp(prev_ori), _dp(motor_cmd),
                                                     _dp(ep_state), _dp(ep_stats), _dp(done), _dp(done_list), _dp(done_count)))

    def set_stage_reset(self, binding=None, **fields):
        """Bind the stages with memory (ground, estimator, gait, walk gait, swing update, stance update / tick, pose plan, MPC front-end) to a device
        mask and a device tick count: binding = stage_reset(...), or its fields as keywords.  A masked robot is reset at its next stage calls
        (a non-zero scalar reset of a call still wins), and with ticks the gaits and the stance stage run on the robot's own clock.  The arrays
        are read when the kernels run.  Loop: episode step, plant step, ground, estimator, gait, swing, front-end or stance, tick."""
        b = stage_reset(**fields) if binding is None else binding
        self._chk(self._lib.qrgpu_set_stage_reset(self._h, C.byref(b)))

    def clear_stage_reset(self):
        self._chk(self._lib.qrgpu_set_stage_reset(self._h, None))

    def observe_state_rows(self, desc):
        """Rows of obs_state for desc: OBSERVE_STATE_ROWS, or OBSERVE_STATE_ROWS_MV with the motor-velocity window."""
        return self._lib.qrgpu_observe_state_rows(C.byref(desc))

    def observe_batch(self, n, desc, raw, obs_state, est_in, rpy, ground_in=None, tick=None, est_out_prev=None, reset=False, step=0):
        """qrRobot*::ReceiveObservation of n robots (desc: observe_desc()): raw [41][n] = rows 0-40 as a plant call writes them -> the filtered rows
        0-40 of est_in [54][n] (may be raw itself), rpy [3][n], ground_in [23][n] and tick [n] uint32 (both optional) for ground_update_batch,
        estimator_update_batch and pack_state_batch.  obs_state [observe_state_rows(desc)][n] float32 is the stage's memory, zero = fresh; reset
        starts every robot afresh, and a stage-reset binding's mask does so per robot.  est_out_prev [42][n]: the estimator's output of the
        previous tick (None: the base position is (0, 0, base_height)).  step: the caller's loop count, the sensor noise's counter."""
        self._chk(self._lib.qrgpu_observe_batch(self._h, n, C.byref(desc), int(bool(reset)), int(step) & 0xffffffff, _dp(raw), _dp(est_out_prev),
                                                _dp(obs_state), _dp(est_in), _dp(rpy), _dp(ground_in), _dp(tick)))

    def command_update(self, n, desc, joy, cmd_state, state_des=None, fe_in=None, fh_in=None, swing_vel_in=None, stance_cmd=None, reset=0):
        """qrDesiredStateCommand::Update of n robots (desc: command_desc()): joy [JOY_ROWS][n] = joyCmdVx, Vy, Vz, RollRate, PitchRate, YawRate,
        joycmdBodyHeight, joyCtrlState (an RC_* value) -> state_des [12][n] and the rows the other stages read: fe_in 0-5, fh_in 16-20, swing_vel_in
        23-26, stance_cmd 0-6 (each optional).  cmd_state [CMD_STATE_ROWS][n] is the filter's memory; reset 1 starts every robot from zeros, a
        stage-reset binding's mask does so per robot."""
        self._chk(self._lib.qrgpu_command_update_batch(self._h, n, C.byref(desc), int(reset), _dp(joy), _dp(cmd_state), _dp(state_des), _dp(fe_in), _dp(fh_in),
                                                       _dp(swing_vel_in), _dp(stance_cmd)))

    def trot_inputs(self, n, est_in, est_out, rpy, gait_out, gait_state=None, fe_in=None, fh_in=None, swing_in=None, est_in_next=None):
        """The getters between the trot's stages: fe_in rows 6-25 and 38-41, fh_in 21-45, swing_in 36-57 and rows 41-44 of est_in_next (usually
        est_in itself) from est_in, est_out, rpy [3][n], gait_out [24][n] and gait_state (needed with fe_in).  Each output is optional."""
        self._chk(self._lib.qrgpu_trot_inputs_batch(self._h, n, _dp(est_in), _dp(est_out), _dp(rpy), _dp(gait_out), _dp(gait_state), _dp(fe_in), _dp(fh_in),
                                                    _dp(swing_in), _dp(est_in_next)))

    def mpc_command(self, n, desc, tau, qdes, swing_in, gait_out, gait_state, cmd_mem, motor_cmd, reset=0):
        """The motor command of the MPC mode (desc: mpc_command_desc()): motor_cmd [60][n] = p, Kp, d, Kd, tua from the tick's tau [12][n], the swing
        targets qdes [24][n], rows 0-3 of swing_in, gait_out and gait_state.  cmd_mem [1][n] int32: the legs with a swing entry, bit per leg; reset
        1 clears it for every robot, a stage-reset binding's mask per robot."""
        self._chk(self._lib.qrgpu_mpc_command_batch(self._h, n, C.byref(desc), int(reset), _dp(tau), _dp(qdes), _dp(swing_in), _dp(gait_out), _dp(gait_state),
                                                    _dp(cmd_mem), _dp(motor_cmd)))

    def velocity_inputs(self, n, est_in, est_out, gait_out, gait_state, state_des, ground_out=None, swing_vel_in=None, est_in_next=None, cmd_mem=None,
                        swing_flag=None, terrain=0, reset=0):
        """The getters between the stages of the force-balance trot (mode VELOCITY): swing_vel_in rows 0-7 and 20-52 (rows 8-19 are
        swing_update_batch's), rows 41-44 of est_in_next (usually est_in itself), cmd_mem [1][n] int32 (the legs with a swing entry, bit per leg; reset
        1 clears it for every robot, a stage-reset binding's mask per robot) and swing_flag [4][n] for stance_tick_batch, whose swing_q is row 24 of
        swing_velocity_batch's output.  ground_out is read on terrain >= 2 alone.  Each output is optional; swing_flag needs cmd_mem."""
        self._chk(self._lib.qrgpu_velocity_inputs_batch(self._h, n, int(terrain), int(reset), _dp(est_in), _dp(est_out), _dp(ground_out), _dp(gait_out),
                                                        _dp(gait_state), _dp(state_des), _dp(swing_vel_in), _dp(est_in_next), _dp(cmd_mem), _dp(swing_flag)))

    def fsm_state_rows(self):
        """Rows of fsm_state, the control state machine's memory (float32; the first fsm_update on new arrays is a reset)."""
        return FSM_STATE_ROWS

    def fsm_update(self, n, desc, fsm_state, joy, plan, stage_mask=None, joy_msg=None, script=None, n_script=0, ticks=None, done=None, bits=EP_REASONS,
                   reset=0):
        """The head of a robot's tick (desc: fsm_desc()): JoyCallback from joy_msg [JOY_MSG_ROWS][n] (row 0: a message arrived; buttons A, B, X, Y, RB;
        axes [0], [3], [4]; gaitSwitch) or from the device script [FSM_SCRIPT_ROWS][n_script] (tick, JOY_BTN_* mask, the three axes) keyed on ticks [n]
        (row 0 of ep_state), the change-request block of Update, RunFSM up to the decision -> joy [JOY_ROWS][n] for command_update, plan [n] int32
        (FSM_PLAN_* bits) and stage_mask [n] int32 = (done & bits) | FSM_ENTERED for set_stage_reset.  reset, or a robot with done & bits, starts
        as constructed."""
        self._chk(self._lib.qrgpu_fsm_update_batch(self._h, n, C.byref(desc), int(reset), _dp(joy_msg), _dp(script), int(n_script), _dp(ticks), _dp(done),
                                                   int(bits) if done is not None else 0, _dp(fsm_state), _dp(joy), _dp(plan), _dp(stage_mask)))

    def fsm_zero_command(self, n, plan, state_des=None, fe_in=None, fh_in=None, swing_vel_in=None, stance_cmd=None):
        """stateDes.segment(6, 6) = 0 of SwitchMode / StandLoop for the robots whose plan has FSM_PLAN_PHASE1, after command_update: state_des rows 6-11,
        fe_in 3-5, fh_in 16-19, swing_vel_in 23-26, stance_cmd 1-6 (each optional)."""
        self._chk(self._lib.qrgpu_fsm_zero_command_batch(self._h, n, _dp(plan), _dp(state_des), _dp(fe_in), _dp(fh_in), _dp(swing_vel_in), _dp(stance_cmd)))

    def fsm_command(self, n, desc, plan, est_in, motor_cmd_loco, fsm_state, motor_cmd, fsm_out=None):
        """The rest of RunFSM: every robot's motor_cmd [60][n] column chosen by its plan (the locomotion column motor_cmd_loco passed through, the stand
        blend, an action tick, the hold, zeros, or the previous tick's), iter, OnExit / OnEnter, the torque clip; fsm_out [FSM_OUT_ROWS][n] reports the
        state.  motor_cmd_loco may be motor_cmd itself."""
        self._chk(self._lib.qrgpu_fsm_command_batch(self._h, n, C.byref(desc), _dp(plan), _dp(est_in), _dp(motor_cmd_loco), _dp(fsm_state), _dp(motor_cmd),
                                                    _dp(fsm_out)))

    def mode_route(self, n, desc, mode_sel, chain, plan=None, route_flags=None, chain_count=None):
        """The chain each robot is on this tick (desc: mode_route_desc()): chain [n] int32 = CHAIN_NONE, CHAIN_MPC or CHAIN_FORCE_BALANCE from mode_sel [n]
        float32 (row 45 of fsm_state; read at every call) and plan [n] int32 (optional: a robot whose plan has neither FSM_PLAN_RUN nor FSM_PLAN_PHASE1
        is on no chain).  A mode that is no mode sets ROUTE_BAD_MODE in route_flags [n] int32, a mode without a chain ROUTE_NO_CHAIN; both run on
        desc.fallback_chain.  chain_count [3] int32: the robots per chain."""
        self._chk(self._lib.qrgpu_mode_route_batch(self._h, n, C.byref(desc), _dp(mode_sel), _dp(plan), _dp(chain), _dp(route_flags), _dp(chain_count)))

    def set_mode_route(self, chain):
        """Bind chain [n] int32 (mode_route's output; read when the kernels run): tick_cadence_batch then solves only the robots on CHAIN_MPC, and
        stance_tick_batch, vmc_force_batch and vmc_force_world_batch only those on CHAIN_FORCE_BALANCE; every output column of any other robot stays as
        it was.  Every other call ignores the binding."""
        self._chk(self._lib.qrgpu_set_mode_route(self._h, _dp(chain)))

    def clear_mode_route(self):
        self._chk(self._lib.qrgpu_set_mode_route(self._h, None))

    def mode_command(self, n, chain, cmd_mpc, cmd_fb, motor_cmd, status_mpc=None, status_fb=None, status=None):
        """Every robot's motor_cmd [60][n] column and status word from its own chain: cmd_mpc / status_mpc where chain is CHAIN_MPC, cmd_fb / status_fb
        where it is CHAIN_FORCE_BALANCE, zeros otherwise; bit for bit.  motor_cmd may be either input.  fsm_command follows and reads motor_cmd as
        its motor_cmd_loco."""
        self._chk(self._lib.qrgpu_mode_command_batch(self._h, n, _dp(chain), _dp(cmd_mpc), _dp(cmd_fb), _dp(status_mpc), _dp(status_fb), _dp(motor_cmd),
                                                     _dp(status)))

    def mpc_frontend_batch(self, n, fe_in, fe_state, traj, gait, wbc_cmd=None, mpc_updated=None, num_horizon_l=2, dt_ctrl=0.002, dt_mpc=0.06):
        """SetupCommand + Run + UpdateMPC (without the solve) of n robots: qr_mpc_stance_leg_controller.cpp:158-382."""
        self._chk(self._lib.qrgpu_mpc_frontend_batch(self._h, n, int(num_horizon_l), float(dt_ctrl), float(dt_mpc), _dp(fe_in), _dp(fe_state),
                                                     _dp(traj), _dp(gait), _dp(wbc_cmd), _dp(mpc_updated)))

    def mpc_assemble_batch(self, n, mpc_state, traj, gait, H, g, type_id=None):
        self._chk(self._lib.qrgpu_mpc_assemble_batch(self._h, n, _dp(type_id), _dp(mpc_state), _dp(traj), _dp(gait), _dp(H), _dp(g)))

    def fb_debug_batch(self, n, fb_state, out, type_id=None):
        self._chk(self._lib.qrgpu_fb_debug_batch(self._h, n, _dp(type_id), _dp(fb_state), _dp(out)))

    def set_lpt_schedule(self, on=True):
        """Longest-first workgroup dispatch from the previous call's per-robot solve time (speed only)."""
        self._chk(self._lib.qrgpu_set_lpt_schedule(self._h, 1 if on else 0))

    def set_warm_start(self, on=True):
        """Start each robot slot's active set from its previous solve (speed only; results agree with a cold start to solver tolerance)."""
        self._chk(self._lib.qrgpu_set_warm_start(self._h, 1 if on else 0))

    def set_hessian_mode(self, mode="f32"):
        """K4 arithmetic: "f32" (exact, default) or "bf16x3" (three-limb bf16 on the bf16 matrix cores: BASELINE.json configs[4])."""
        self._chk(self._lib.qrgpu_mpc_set_hessian_mode(self._h, {"f32": 0, "bf16x3": 1}[mode]))

    def set_planned_list(self, on=True, big_nls=0):
        """Robots that needed the rescue pass last call are solved beside the main launch this call (scheduling only)."""
        self._chk(self._lib.qrgpu_set_planned_list(self._h, 1 if on else 0, int(big_nls)))

    def set_rescue_pass(self, on=True):
        self._chk(self._lib.qrgpu_set_rescue_pass(self._h, 1 if on else 0))

    def sync(self):
        self._chk(self._lib.qrgpu_sync(self._h))

    def enable_flop_count(self, on=True):
        self._chk(self._lib.qrgpu_enable_flop_count(self._h, 1 if on else 0))

    def mpc_flop_counts(self):
        """Executed arithmetic of the last counted MPC call, summed over its robots: dict(fp32_vector, fp32_matrix, fp64_sweep, fp64_active_set)."""
        out = (C.c_double * 4)()
        self._chk(self._lib.qrgpu_mpc_flop_counts(self._h, out))
        return dict(fp32_vector=out[0], fp32_matrix=out[1], fp64_sweep=out[2], fp64_active_set=out[3])

    # -- multi-GPU: the all-gather of torques over RCCL (qrgpu_comm.hip) ---------------------------------------------
    def comm_init_rank(self, id_blob, nranks, rank):
        assert len(id_blob) == COMM_ID_BYTES
        self._chk(self._lib.qrgpu_comm_init_rank(self._h, bytes(id_blob), int(nranks), int(rank)))

    def comm_destroy(self):
        self._chk(self._lib.qrgpu_comm_destroy(self._h))

    def allgather_tau(self, tau, n_local, tau_all, slot=0, nccl_comm=None, of_tick=False):
        """Asynchronous on the context's communication stream; tau_all is [nranks][12][n_local] (rank-major).  of_tick: `tau` is what the
        context's last tick_batch produced and nothing queued since writes it (qrgpu_allgather_tau_of_tick: no event on the compute stream)."""
        fn = self._lib.qrgpu_allgather_tau_of_tick if of_tick else self._lib.qrgpu_allgather_tau
        self._chk(fn(self._h, _dp(nccl_comm), _dp(tau), int(n_local), _dp(tau_all), int(slot)))

    def allgather_fence(self, slot=0):
        self._chk(self._lib.qrgpu_allgather_fence(self._h, int(slot)))

    def allgather_wait(self, slot=0):
        """Make the compute stream wait for the gather of `slot` (for a consumer of tau_all queued there); the slot's fence stays due."""
        self._chk(self._lib.qrgpu_allgather_wait(self._h, int(slot)))

    def comm_sync(self):
        self._chk(self._lib.qrgpu_comm_sync(self._h))

    def enable_timing(self, on=True):
        """False: off; True: HIP events around every kernel launch; an int N > 1: around every N-th launch of a kernel; -1: pause."""
        self._chk(self._lib.qrgpu_enable_timing(self._h, int(on) if on is not True else 1))

    def get_timing(self, kernel):
        ms = C.c_double(0); cnt = C.c_int(0)
        self._chk(self._lib.qrgpu_get_timing(self._h, kernel, C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    # -- single-robot host API ------------------------------------------------------------------------
    def mpc_solve1(self, p, v, quat, w, r, rpy, traj, gait, q=None, type_id=0):
        a = [np.ascontiguousarray(x, np.float32) for x in (p, v, quat, w, r, rpy, traj, gait)]
        qa = np.ascontiguousarray(q, np.float32) if q is not None else None
        f = np.zeros(12, np.float64); tau = np.zeros(12, np.float32); st = C.c_int(0)
        self._chk(self._lib.qrgpu_mpc_solve1(self._h, type_id, *[_fp(x) for x in a], _fp(qa) if qa is not None else None,
                                             f.ctypes.data_as(C.POINTER(C.c_double)), _fp(tau), C.byref(st)))
        return f, (tau if q is not None else None), st.value

    def wbc_run1(self, fb_state, wbc_cmd, prev_ori_vel, type_id=0, want_qdes=True):
        s = np.ascontiguousarray(fb_state, np.float32); c = np.ascontiguousarray(wbc_cmd, np.float32)
        prev = np.ascontiguousarray(prev_ori_vel, np.float32).copy()
        tau = np.zeros(12, np.float32); qd = np.zeros(12, np.float32); qdd = np.zeros(12, np.float32); st = C.c_int(0)
        self._chk(self._lib.qrgpu_wbc_run1(self._h, type_id, _fp(s), _fp(c), _fp(prev), _fp(tau),
                                           _fp(qd) if want_qdes else None, _fp(qdd) if want_qdes else None, C.byref(st)))
        return tau, qd, qdd, prev, st.value


class MPCInterface:
    """Drop-in shaped like the free functions of qr_mpc_interface.h (one robot, host pointers).

    The reference keeps its problem in file-static state (qr_mpc_interface.cpp:35-104); here the
    state lives in this object."""

    def __init__(self, ctx=None, type_id=0):
        self.ctx = ctx or Context(max_batch=1)
        self.type_id = type_id
        self._soln = None
        self.status = 0

    def SetupProblem(self, dt, horizon, frictionCoeff, fMax, totalMass, inertia, weight, alpha):
        self.ctx.mpc_setup(self.type_id, float(dt), int(horizon), float(frictionCoeff), float(fMax), float(totalMass),
                           inertia, weight, float(alpha))
        self.horizon = int(horizon)

    def SolveMPCKernel(self, p, v, q, w, r, rpy, state_trajectory, gait):
        """r: 3x4 (column = leg) as Eigen::Matrix<float,3,4>; q: quaternion (w,x,y,z)."""
        r = np.asarray(r, np.float32)
        r_colmajor = r.T.reshape(12) if r.shape == (3, 4) else r.reshape(12)
        f, _, st = self.ctx.mpc_solve1(p, v, q, w, r_colmajor, rpy, np.asarray(state_trajectory, np.float32)[:12 * self.horizon],
                                       np.asarray(gait, np.float32)[:4 * self.horizon], None, self.type_id)
        self._soln, self.status = f, st

    def GetMPCSolution(self, index):
        """First-step forces only (indices 0..11), as every call site of the reference uses it
        (qr_mpc_stance_leg_controller.cpp:404); 0 before the first solve (qr_mpc_interface.cpp:448)."""
        if self._soln is None:
            return 0.0
        return float(self._soln[index])


class WbcLocomotionController:
    """Shaped like qrWbcLocomotionController<float> (QI/controllers/wbc/qr_wbc_locomotion_controller.hpp:47-59).

    Run() keeps the reference's cadence: it computes on every 2nd call (iteration % 2 == 0,
    qr_wbc_locomotion_controller.cpp:111,133) and otherwise re-applies the last torques to the
    stance legs (UpdateLegCMD runs every call, :129)."""

    def __init__(self, ctx, type_id=0):
        self.ctx, self.type_id = ctx, type_id
        self.iteration = 0
        self.prev_ori_vel = np.zeros(3, np.float32)
        self.jointTorqueCmd = np.zeros(12, np.float32)
        self.desiredJPos = np.zeros(12, np.float32)
        self.desiredJVel = np.zeros(12, np.float32)
        self.status = 0

    def Run(self, fb_state, wbc_cmd, leg_cmd_tua):
        """leg_cmd_tua: array of 12 torques, stance-leg entries are overwritten in place."""
        if self.iteration % 2 == 0:
            tau, qd, qdd, prev, st = self.ctx.wbc_run1(fb_state, wbc_cmd, self.prev_ori_vel, self.type_id)
            self.jointTorqueCmd, self.desiredJPos, self.desiredJVel, self.prev_ori_vel, self.status = tau, qd, qdd, prev, st
        contact = np.asarray(wbc_cmd, np.float32)[63:67]
        for leg in range(4):
            if contact[leg] != 0:
                leg_cmd_tua[3 * leg:3 * leg + 3] = self.jointTorqueCmd[3 * leg:3 * leg + 3]
        self.iteration += 1
        return leg_cmd_tua
