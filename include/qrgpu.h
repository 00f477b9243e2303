/* ============================================================================
 * qrgpu.h -- C ABI of libqrgpu.so: batched convex-MPC + WBC control ticks for
 * quadrupeds on AMD MI355X (gfx950).  Plain pointers and sizes only; no C++,
 * torch or HIP types appear in any signature (the stream is passed as void*).
 *
 * Each entry point replaces one seam of TopHillRobotics/quadruped-robot
 * ("QI/" = quadruped/include/quadruped/, "QS/" = quadruped/src/):
 *
 *   qrgpu_mpc_setup        <- Quadruped::SetupProblem          QI/controllers/mpc/qr_mpc_interface.h:157
 *   qrgpu_mpc_solve1       <- Quadruped::SolveMPCKernel + 12x GetMPCSolution   :200, :215
 *   qrgpu_mpc_solve_batch  <- the same, for n independent robots (MPCStanceLegController::SolveDenseMPC
 *                             + GetAction torque map, QS/controllers/mpc/qr_mpc_stance_leg_controller.cpp:385-410,129-156)
 *   qrgpu_wbc_setup        <- qrRobot*::BuildDynamicModel + qrWbcLocomotionController ctor gains
 *                             QS/robots/qr_robot_a1_sim.cpp:176-343, QS/controllers/wbc/qr_wbc_locomotion_controller.cpp:29-77
 *   qrgpu_wbc_run1         <- qrWbcLocomotionController<float>::Run   QI/controllers/wbc/qr_wbc_locomotion_controller.hpp:59
 *   qrgpu_wbc_run_batch    <- the same, for n robots
 *   qrgpu_mpc_frontend_batch <- MPCStanceLegController::SetupCommand/Run/UpdateMPC (reference trajectory + contact table)
 *                             QS/controllers/mpc/qr_mpc_stance_leg_controller.cpp:158-382
 *   qrgpu_vmc_setup / qrgpu_vmc_force_batch / qrgpu_vmc_force_world_batch <- Quadruped::ComputeContactForce (control-frame and world-frame
 *                             overloads, :190-301, :304-398) + qrRobot::MapContactForceToJointTorques
 *                             QS/controllers/balance_controller/qr_qp_torque_optimizer.cpp:190-301, QS/robots/qr_robot.cpp:241-251
 *                             (what TorqueStanceLegController::GetAction calls, qr_torque_stance_leg_controller.cpp:500-507)
 *   qrgpu_estimator_update_batch <- qrRobot::UpdateDataFlow (leg kinematics) + qrRobotVelocityEstimator::Update + qrRobotPoseEstimator::Update
 *                             QS/robots/qr_robot.cpp:62-72,187-197, QS/estimators/qr_robot_velocity_estimator.cpp:77-133,
 *                             QS/estimators/qr_robot_pose_estimator.cpp:68-165 (qrRobotEstimator::Update, qr_robot_estimator.cpp:79-83)
 *   qrgpu_gait_update_batch <- qrOpenLoopGaitGenerator::Update / Schedule   QS/gait/qr_openloop_gait_generator.cpp:126-249
 *   qrgpu_swing_targets_batch <- qrRaibertSwingLegController::GetAction (ADVANCED_TROT)   QS/controllers/qr_swing_leg_controller.cpp:362-424
 *   qrgpu_footholds_batch  <- qrRaibertSwingLegController::Update + qrFootholdPlanner::ComputeHeuristicFootHold
 *                             QS/controllers/qr_swing_leg_controller.cpp:211-236, QS/planner/qr_foothold_planner.cpp:110-239
 *   qrgpu_pose_plan_batch     <- qrPosePlanner::Update (SQP) + ResetBasePose                       QS/planner/qr_pose_planner.cpp
 *   qrgpu_stance_update_batch <- TorqueStanceLegController::UpdateFRatio + UpdateDesCommand   QS/controllers/balance_controller/
 *                             qr_torque_stance_leg_controller.cpp:89-172, 174-477 (with qrComAdjuster::Update, QS/planner/qr_com_adjuster.cpp:61-108,
 *                             and qrPosePlanner::GetIntermediateBasePose, QI/planner/qr_pose_planner.h:327-365)
 *   qrgpu_stance_command_batch <- the motor-command tail of TorqueStanceLegController::GetAction (:503-541) + qrLocomotionController::GetAction's
 *                             merge with the swing command   QS/controllers/qr_locomotion_controller.cpp:128-147
 *   qrgpu_stance_tick_batch <- TorqueStanceLegController::GetAction (:480-545) + that merge: front-end, force-balance QP, motor commands
 *   qrgpu_velocity_inputs_batch <- the reads of the velocity mode's controllers between those stages (the force-balance trot, JOY_TROT): swingFootIds,
 *                             the inputs of qrRaibertSwingLegController::GetAction's VELOCITY case and the keys of swingJointAnglesVelocities with the
 *                             command loop's flag   QS/controllers/qr_swing_leg_controller.cpp:100, 218-229, 256-276, 294, 306, 408-424, 446-448
 *   qrgpu_tick_batch       <- one MPC solve + one WBC tick per robot, WBC fed with that MPC's Fr_des
 *                             (QS/fsm/qr_fsm_state_locomotion.cpp:130-158 without the MPC/WBC time-slicing)
 *   qrgpu_tick_cadence_batch <- the same state WITH the time-slicing: per robot the MPC on the ticks that re-plan, the held force through the
 *                             current Jacobian and the WBC on every other tick (wbcData.allowAfterMPC), from a device mask
 *   qrgpu_set_torque_epilogue <- the motor-command tail of that state: abad compensation (:141-151) and the +-23 N m clip
 *                             (QS/fsm/qr_safety_checker.cpp:48-66)
 *   qrgpu_comm_* / qrgpu_allgather_tau <- no reference equivalent (the reference runs one robot per process): the all-gather of torques
 *                             of BASELINE.json's sharded configurations
 *
 * Error behaviour mirrors the reference: no exceptions; the reference prints
 * "failed to solve!" and carries on (qr_mpc_interface.cpp:440-442) -- here every
 * robot gets a status word instead and every call returns a qrgpu_error.
 *
 * All computation runs in hand-written HIP kernels.  There is NO CPU fallback:
 * without a usable gfx950 device qrgpu_create fails with QRGPU_ERR_NO_DEVICE.
 *
 * Batched layouts are structure-of-arrays, [field][robot] with the robot index
 * fastest (array element (f, i) at f*n + i), float32, device memory:
 *   mpc_state [28][n] : p[3], v_world[3], quat_wxyz[4], w_world[3], r[12] (3x4 column-major:
 *                       r[3*leg+axis], foot - CoM in the world-aligned frame), rpy[3]
 *   traj      [12h][n]: desired state per horizon step (rpy, xyz, omega, v), step-major
 *   gait      [4h][n] : contact table, step-major (row-major h x 4, as mpcTable)
 *   fb_state  [37][n] : quat_wxyz[4], pos[3], omega_body[3], v_body[3], q[12], qd[12]   (FBModelState)
 *   wbc_cmd   [67][n] : pBody_des[3], vBody_des[3], aBody_des[3], pBody_RPY_des[3], vBody_Ori_des[3],
 *                       pFoot_des[12], vFoot_des[12], aFoot_des[12], Fr_des[12], contact[4] (0/1)  (qrWbcCtrlData)
 *   prev_ori  [3][n]  : in/out, desiredVel of the body-orientation task from the previous WBC call
 *                       (stateful quirk of task_set/qr_task_body_orientation.cpp:68 vs :73)
 *   force     [12][n] : MPC ground-reaction forces of horizon step 0, world frame (= wbcData.Fr_des)
 *   tau       [12][n] : joint torques
 *   vmc_in    [37][n] : force-balance QP inputs: footPositionsInBaseFrame[12] (3*leg+axis), desiredAcc[6], contacts[4],
 *                       Rcb[9] (row-major; identity on PLANE / PLUM_PILES terrain), g.head(3) ((0,0,9.8) on a plane), surfaceNormal[3]
 *   est_in    [54][n] : estimator inputs: baseAccInBaseFrame[3], baseLinearAcceleration[3], quat_wxyz[4], rpyRate[3], footContact[4],
 *                       motor angles q[12], motor velocities dq[12], desiredLegState[4] (LegState values), groundOrientationMat[9]
 *                       (GetAlignedDirections, row-major; identity on a plane)
 *   est_out   [42][n] : filtered baseLinearAcceleration[3], baseVInWorldFrame[3], baseVelocityInBaseFrame[3], baseWInWorldFrame[3],
 *                       footPositionsInBaseFrame[12], footVelocitiesInBaseFrame[12] (3*leg+axis), basePosition[3] (odometry x, y and
 *                       the stance-foot height), heightInControlFrame (NaN = unchanged: no stance foot), absoluteHight, odometry yaw
 *   fe_in     [64][n] : front-end inputs per control tick: des_height, des_roll, des_pitch, x_vel_cmd, y_vel_cmd, yaw_vel_cmd
 *                       (stateDes 2,3,4,6,7,11 after UpdateDesCommand), basePosition[3], yaw, quat_wxyz[4], footPosWorld[12]
 *                       (leg-major), footTargetPositionsInWorldFrame[12], contacts[4], phaseInFullCycle[4], dutyFactor[4],
 *                       normalizedPhase[4], desiredLegState[4], legState[4] (LegState enum values as floats),
 *                       firstSwingBaseState x, y
 *   fe_state  [8][n]  : in/out controller memory: xVelDes, yVelDes, yawTurnRate, yawDesTrue, posDesiredinWorld[3], iterationCounter
 *
 * ENVIRONMENT SWITCHES.  These are the supported ones (read once per process).  qrgpu_create warns once about any other QRGPU_* variable it
 * finds: the launch forms kept for a test or a profiling run are laboratory switches, ignored unless QRGPU_LAB=1 is set (LAB_NOTES.md A.1
 * lists them, and the retired ones with what each measured).
 *   name                    default  effect
 *   QRGPU_TICK_PIPELINE     1        0: qrgpu_tick_batch queues the WBC launch behind the MPC launches (the serial tick) whatever qrgpu_set_tick_pipeline says
 *   QRGPU_PIPE_GATE_MS      50       bound of the gate in front of a pipelined tick's WBC launch; one that gives up turns the tick into the serial one
 *   QRGPU_PLAN_GO_MS        50       bound of the planned launch's wait for its "go"; one that gives up calls the plan off for the call
 *   QRGPU_PIPE_WAIT_US      4000     bound of a WBC workgroup's wait for its robot's forces (then QRGPU_ST_PIPE_TIMEOUT)
 *   QRGPU_OV_WAIT_US        20000    overlapped ticks: bound of a robot's waits for its previous solve / WBC pass (then QRGPU_ST_PIPE_TIMEOUT)
 *   QRGPU_OV_PLAN_HOLD      31       overlapped ticks: calls on the plain pipelined tick after a lane found a planned list (0: never go back)
 *   QRGPU_OV16              1        overlapped ticks: 0 keeps contexts with a horizon beyond 11 on the plain pipelined tick
 *   QRGPU_OV_FAULT          0        test hooks of the give-up paths (tests/test_gpu_overlap.py): 1 makes every chained tick wait for an epoch nobody writes;
 *                                    2 (h > 11) sends the planned launch's workgroups home without the robots the main pass hands on
 *   QRGPU_COMM_EVENTS       unset    the all-gather's hand-overs: unset = stream events when the communicator has more than one rank, polled counts
 *                                    with one; 1 = events always; 0 = polled counts always
 *   QRGPU_SINGLE_COPIES     0        1: the single-robot calls stage through device buffers and three copies instead of one mapped pinned block
 *   QRGPU_PERSIST           1        h > 11: persistent main pass (one workgroup per resident slot taking robots off per-XCD queues); 0 off, 2 also at h <= 11
 *   QRGPU_H16_TWO           1        h > 11: two workgroups per CU from 3.5 robots per CU on; 0 never, 2 from 64 robots on
 *   QRGPU_H16_TWO_HOLD      31       ... calls on one workgroup per CU after the planned list outgrew 45 % of the batch
 *   QRGPU_H16_BIG_US        450      ... smoothed solve time from which a robot is planned onto a whole CU
 *   QRGPU_H16_BIG_STAY_US   300      ... and below which it leaves it again
 *   QRGPU_LIB               unset    (Python mirror, bench.py) path of another build of libqrgpu.so to load: A/B runs
 *   QRGPU_EXTRA_FLAGS       unset    (build.py) extra hipcc flags; -DQR_TIMELINE builds the per-tick stamps of qrgpu_debug_timeline in
 *   QRGPU_LAB               0        1: the laboratory switches are read
 *   GPU_MAX_HW_QUEUES       (HIP)    the HIP runtime's: hardware queues per process (its default 4; the Python mirror sets 8 when unset).  Streams that
 *                                    share a queue serialise each other: qrgpu_set_tick_overlap probes for it and refuses the mode
 * ========================================================================== */
#ifndef QRGPU_H
#define QRGPU_H

#ifdef __cplusplus
extern "C" {
#endif

#define QRGPU_MAX_HORIZON 16      /* K_MAX_GAIT_SEGMENTS, QI/controllers/mpc/qr_mpc_interface.h:33 */
#define QRGPU_MAX_TYPES   4       /* robot types (parameter sets) per context */

typedef struct qrgpu_ctx qrgpu_ctx;

typedef enum {
    QRGPU_OK = 0,
    QRGPU_ERR_NO_DEVICE = 1,      /* no gfx950 device / HIP runtime failure at create */
    QRGPU_ERR_BAD_ARG = 2,
    QRGPU_ERR_NOT_SETUP = 3,      /* solve before setup */
    QRGPU_ERR_LAUNCH = 4,         /* kernel launch or runtime error (see qrgpu_last_error) */
    QRGPU_ERR_ALLOC = 5,
    QRGPU_ERR_COMM = 6            /* RCCL failure (librccl missing, communicator error; see qrgpu_last_error) */
} qrgpu_error;

/* Per-robot status word written by the kernels: bits 0-7 and 24-31 are the flags below (0 = converged), bits 8-23
 * hold the number of MPC active-set iterations (diagnostic).  Test `(status & QRGPU_ST_FLAG_MASK) == 0`. */
#define QRGPU_ST_FLAG_MASK     0xff0000ffu
#define QRGPU_ST_ITERATIONS(s) (((s) >> 8) & 0xffff)
#define QRGPU_ST_OK            0
#define QRGPU_ST_MPC_MAXITER   0x1    /* active-set iteration cap reached            */
#define QRGPU_ST_MPC_INFEAS    0x2    /* no feasible step for a violated row, or the solve ended with a row it had set aside as
                                         dependent violated, or an active row not tight, by more than 1e-4 N: the forces are not the optimum */
#define QRGPU_ST_MPC_OVERFLOW  0x4    /* working set outgrew its LDS allotment       */
#define QRGPU_ST_MPC_NOTSPD    0x8    /* Hessian pivot <= 0                          */
#define QRGPU_ST_BAD_TYPE      0x01000000  /* d_type_id names a type outside [0, QRGPU_MAX_TYPES) or one that was never set up: the robot was
                                         computed with the first type that was set up and its result must not be used */
#define QRGPU_ST_PIPE_TIMEOUT  0x02000000  /* pipelined tick: the WBC never saw this robot's MPC forces arrive; the torques must not be used */
#define QRGPU_ST_WBC_MAXITER   0x10
#define QRGPU_ST_WBC_INFEAS    0x20
#define QRGPU_ST_VMC_MAXITER   0x40
#define QRGPU_ST_VMC_INFEAS    0x80   /* QuadProg++ would have returned +inf (e.g. the 1e-7 window of a swing foot, qr_qp_torque_optimizer.cpp:79-81);
                                         the force is the iterate QuadProg++ stops at, which is what the reference goes on to use (:281-297).
                                         On up to 0.7 % of the ticks of a measured batch (three stance feet on a pitched normal, friction 0.55
                                         and more; none in 3 000 ticks at the default 0.5, none in 2 000 on level ground at 0.9) that iterate
                                         is decided by the rounding inside QuadProg++ and can be 1e6 .. 5e9 N: there only this flag is
                                         guaranteed, and the force returned is finite and of the order of the robot's weight (DESIGN.md 4.6,
                                         LAB_NOTES A.9, tests/golden/vmc_grid_golden.npz well_posed) */

/* What BuildDynamicModel reads from YAML plus what the WBC controller hard-codes.
 * Defaults (qrgpu_model_desc_default) are the A1 values. */
typedef struct {
    float hip_l, upper_l, lower_l;        /* robot_params.hip_l / upper_l / lower_l          */
    float body_size[3];                   /* robot_params.body_size (unused by the torque path) */
    float kp_body_pos, kd_body_pos;       /* 100 / 10   qr_wbc_locomotion_controller.cpp:62-63 */
    float kp_body_ori, kd_body_ori;       /* 100 / 10   :66-67 */
    float kp_foot, kd_foot;               /* 500 / 10   :70-71 */
    float weight_fb, weight_fr;           /* 0.1 / 1    :44-45 */
    float mu;                             /* 0.4        QS/controllers/wbc/qr_single_contact.cpp:34 */
} qrgpu_model_desc;

void qrgpu_model_desc_default(qrgpu_model_desc *d);

/* Per-type constants of the force-balance (VMC) QP: ComputeContactForce's non-per-tick arguments.  Defaults: A1 + the header defaults
 * (QI/controllers/balance_controller/qr_qp_torque_optimizer.h:144-153), acc_weight of config/a1_sim/stance_leg_controller.yaml.
 * friction: 0.5 is the control-frame overload's default (:144-153).  The world-frame overload's own default is 0.6
 * (qr_qp_torque_optimizer.h:171-182), and TorqueStanceLegController::GetAction passes none (qr_torque_stance_leg_controller.cpp:496-498):
 * a type that stands for that call is set up with friction = 0.6. */
typedef struct {
    float mass;                           /* robot->totalMass */
    float inertia[9];                     /* robot->totalInertia, Eigen column-major (the YAML list as mapped by MatrixXf::Map) */
    float acc_weight[6];
    float reg_weight, friction, fmin_ratio, fmax_ratio;   /* 1e-4, 0.5, 0.01, 10 */
    float hip_l, upper_l, lower_l;        /* leg geometry for the J^T f torque map */
} qrgpu_vmc_desc;
void qrgpu_vmc_desc_default(qrgpu_vmc_desc *d);

/* ---- lifetime -------------------------------------------------------------- */
/* device_id: HIP device ordinal.  max_batch: largest n of any batched call. */
int  qrgpu_create(int device_id, int max_batch, int horizon_max, qrgpu_ctx **out);
void qrgpu_destroy(qrgpu_ctx *ctx);
/* The compute stream: every batched call is queued on it and completes in its order.  A context starts with a non-blocking stream of its own
 * (qrgpu_get_stream hands it out, for a caller that wants to queue its own work in order with the library's); qrgpu_set_stream names another
 * hipStream_t -- NULL = the default (null) stream, on which several contexts of one process serialise each other's launches. */
int  qrgpu_set_stream(qrgpu_ctx *ctx, void *hip_stream);
void *qrgpu_get_stream(qrgpu_ctx *ctx);
/* Longest-first dispatch of the batched MPC solve (default on): robot i's solve time in one call orders the workgroup
 * dispatch of the next call with the same n (control ticks are temporally coherent).  Scheduling only -- results do not
 * depend on it; a batch whose robots were reshuffled between calls merely loses the speed-up.  Turning it on or off
 * forgets the history. */
int  qrgpu_set_lpt_schedule(qrgpu_ctx *ctx, int on);
/* Warm start of the batched MPC solve (default on): robot slot i's final working set in one call (by leg-step, realigned to the scrolling
 * contact table) is where its solve starts in the next call with the same n -- the equality-constrained problem on that set is solved in
 * one block instead of adding its rows one active-set iteration at a time; rows that no longer belong leave, missing ones are added.  The
 * reference cold-starts qpOASES at every solve (QProblem::init, qr_mpc_interface.cpp:430); the QP has one optimum, so results agree
 * with a cold start to the solver's tolerance (1e-9 relative) -- not bit for bit: switch it off where run-to-run bit identity across a
 * changing history matters.  Turning it on or off forgets what is stored. */
int  qrgpu_set_warm_start(qrgpu_ctx *ctx, int on);
/* Planned list of the batched MPC solve (default on, big_nls = 0): a robot that needed the rescue pass in one call -- or ended within a few
 * rows of the main pass's LDS allotment -- is solved in the NEXT call with the same n by a list launch of its own (whole CU's LDS, 96
 * working-set positions), issued at the start of the call on a second stream of the context beside the main launch, which skips it: the
 * batch no longer waits for a re-solve after the main launch.  big_nls > 0 additionally sends every robot with at least that many stance
 * leg-steps (4h = all feet down over the whole horizon) there.  Scheduling -- with two things a caller may see: the list launches are other
 * instantiations of the kernel than the main pass (whole CU's LDS, 96 working-set positions), so a robot's forces agree between the two to the
 * solver's tolerance (1e-6 of the largest force; the QP has one optimum), not bit for bit; and a robot at the very edge of what a launch can
 * hold may carry QRGPU_ST_MPC_OVERFLOW under one schedule and not under the other (tests/test_gpu_wbc.py allows two such robots in 1024 between
 * the serial and the pipelined tick).  A robot the main pass solves under both schedules has the same bits.
 * The host learns the list's length through pinned memory without a sync; so that a caller which queues calls faster than the GPU runs
 * them still gets its first plans, the first two batched calls after the history was reset (a new n, qrgpu_set_lpt_schedule) end with a
 * hipStreamSynchronize on the context's stream.  Every later call stays asynchronous.
 * At h > 11 and 3.5 robots per CU or more the main pass runs two workgroups per CU on half the LDS each, and the list is also where the robots
 * go whose inverse Hessian does not fit half a CU (43 stance leg-steps and more at h = 16; a smaller big_nls of the caller's stands) and those
 * whose solves are the longest of the tick; with the planned list, the rescue pass or the longest-first schedule switched off such batches
 * run one workgroup per CU.  The same two caveats apply. */
int  qrgpu_set_planned_list(qrgpu_ctx *ctx, int on, int big_nls);
/* Rescue pass of the batched MPC solve (default on).  A working set that outgrows the 64 lanes of the four-wave loop is handed over
 * in place to the single-wave loop (up to 96 rows) -- that needs no switch.  What remains are robots limited by LDS (an all-stance inverse
 * Hessian at h = 10 leaves room for 56 rows): they are re-solved by the same kernel with the whole CU's LDS in a second, normally
 * empty launch, at most 64 robots per call (the rest keep QRGPU_ST_MPC_OVERFLOW), h <= 11 and the two-workgroups-per-CU main pass of h > 11 (otherwise at h > 11 such robots keep S^-1 in a global scratch instead).
 * A robot nothing can hold keeps QRGPU_ST_MPC_OVERFLOW. */
int  qrgpu_set_rescue_pass(qrgpu_ctx *ctx, int on);
/* Pipelined tick (default on; batches of 64 robots and more): qrgpu_tick_batch queues its WBC launch on a stream of the context's own
 * BESIDE the MPC launches instead of behind them.  Of a robot's WBC only the relaxation QP at its end reads the MPC's forces, so a WBC
 * workgroup runs dynamics, task set and kinematic projection while its robot's solve is still going and takes the forces when that
 * solve raises the robot's flag; the call's outputs are complete when the context stream's work is (stream order, as before).  Scheduling
 * only: results are those of the serial form bit for bit.  A WBC workgroup that waits longer than 4 ms for its robot (never observed)
 * gives the robot QRGPU_ST_PIPE_TIMEOUT. */
int  qrgpu_set_tick_pipeline(qrgpu_ctx *ctx, int on);
/* Overlapped ticks (default OFF; pipelined ticks): a caller that queues qrgpu_tick_batch calls without waiting for them may let
 * tick t + 1's solves start in the slots tick t's drain leaves empty -- a quarter of a 1024-robot tick's slot-time -- instead of behind tick
 * t's last workgroup.  With the mode on, a tick's launches go on stream sets of the context's own (two, alternating) and the context's stream
 * carries only the tick's join: OUTPUTS ARE COMPLETE IN CALL ORDER ON THE CONTEXT'S STREAM exactly as before (whatever is queued there behind
 * the call sees them), and results are those of the serial tick bit for bit (a robot that goes through a list launch under one schedule and not
 * under the other: to the solver's tolerance, qrgpu_set_planned_list) -- what a robot carries from tick to tick (warm-start words,
 * smoothed cost, the orientation task's memory prev_ori) is handed from its tick-t workgroup to its tick-(t + 1) workgroup behind per-robot
 * epoch words with bounded waits (20 ms; a robot whose wait gives up starts cold and carries QRGPU_ST_PIPE_TIMEOUT).
 * What the caller promises in exchange -- the mode is another contract than "stream order" for the INPUTS:
 *   (1) a tick's input arrays are complete when the call is made, or were produced by work queued on the context's stream BEFORE THE PREVIOUS
 *       qrgpu_tick_batch call: a chained tick does not wait for work queued on the context's stream since then.  Inputs produced there later
 *       (an upload, a front-end kernel) need qrgpu_tick_fence() in front of the tick, which makes that one tick wait for the whole stream;
 *   (2) consecutive ticks write DIFFERENT output arrays (force, tau, qdes, status: double-buffer them) and share prev_ori.  The library
 *       checks this: a tick that reuses any output array of its predecessor, or changes n or prev_ori, or follows any other launch of this
 *       context, is simply not chained -- it waits for the context's stream (an event) and runs as the pipelined tick always did.
 * Throughput, not latency: a chained tick completes LATER after its call than an unchained one (its join waits for a launch that shares the
 * machine with the next tick); bench.py --full prints both beside `value` (config.tick_latency_ms, config.ticks_per_s_no_tick_overlap).
 * Call it AFTER the context's types are set up: the stream sets are made for the horizon the context has at the call (h <= 11: two lanes on the
 * whole machine; h > 11, from 3.5 robots per CU on: two lanes on a machine split by CU masks -- the main pass two to a CU on 192 CUs, the robots
 * that need a whole CU on 64 reserved ones); a context whose horizon changes class afterwards runs plain pipelined ticks until
 * the call is made again.  Throughput of the h > 11 form shows on sequences, not on a handful of ticks: a tick completes about 1.7 periods after
 * its call (1.74 against 1.51 M ticks/s on the mixed h = 16 shard over 25-tick windows, par over 5-tick windows).
 * Needs the context's streams on hardware queues of their own: qrgpu_set_tick_overlap(1) probes that and returns QRGPU_ERR_NOT_SETUP (mode
 * stays off, qrgpu_last_error says why) when two of them share one -- set GPU_MAX_HW_QUEUES=8 in the environment before the process's
 * first HIP call (the HIP runtime's default of 4 is fewer than the streams a context owns). */
int  qrgpu_set_tick_overlap(qrgpu_ctx *ctx, int on);
int  qrgpu_tick_fence(qrgpu_ctx *ctx);
/* How many ticks of this context ran on the overlapped form so far: chained to their predecessor / behind an event of the context's stream. */
int  qrgpu_tick_overlap_stats(const qrgpu_ctx *ctx, int *chained, int *unchained);
const char *qrgpu_last_error(const qrgpu_ctx *ctx);
/* Device facts for reports: returns CU count, writes name (<= len). */
int  qrgpu_device_info(const qrgpu_ctx *ctx, char *name, int len, int *lds_per_cu_bytes);

/* ---- setup (SetupProblem / BuildDynamicModel) -------------------------------
 * A context has ONE horizon (the reference has one global problem size): setting a type up with a different
 * horizon invalidates the MPC setup of the other types until they are set up again with the new horizon. */
int qrgpu_mpc_setup(qrgpu_ctx *ctx, int type_id, float dt, int horizon, float mu, float fmax, float mass,
                    const float inertia[3], const float weights[12], float alpha);
int qrgpu_wbc_setup(qrgpu_ctx *ctx, int type_id, const qrgpu_model_desc *desc);

/* Arithmetic of the Hessian contraction qH = temp * Bqp (K4, qr_mpc_interface.cpp:396-412) of every MPC solve of this context:
 *   QRGPU_HESSIAN_F32     (default) v_mfma_f32_16x16x4_f32: bit for bit the k-ordered fp32 fmaf chain of the reference's dense GEMM;
 *   QRGPU_HESSIAN_BF16X3  BASELINE.json configs[4] ("fp32 QP + bf16 Hessian MFMA"): every fp32 operand cut into three bf16 limbs, the six
 *                         leading cross products per term summed in fp32 by v_mfma_f32_16x16x32_bf16.  H comes out within an ulp or two of the
 *                         exact fp32 assembly (measured 7.5e-9 absolute: the size of the exact H's own asymmetry) but not bit-identical, and on
 *                         this QP an ulp of H is amplified by 1 / (2 alpha), so the mode states ANOTHER QP, a rounding away, and solves that
 *                         one exactly: forces within 1e-5 max(1, |f|) and full-tick torque within 1e-4 max(1, |tau|) of the CPU oracle's solve
 *                         of the very (H, g) this mode assembles, every robot of the configs[4] per-GPU shard
 *                         (tests/test_gpu_mpc.py::test_bf16x3_solve_vs_oracle_on_its_own_hessian).  Against the default mode's answer the
 *                         forces move as the reference's own do between H and H^T.  The default stays QRGPU_HESSIAN_F32 for every
 *                         configuration, configs[4] included: it is bit-exact against the reference's fp32 GEMM AND faster here (the limb
 *                         cuts dominate the operand generation); this mode exists because that configuration names it. */
#define QRGPU_HESSIAN_F32    0
#define QRGPU_HESSIAN_BF16X3 1
int qrgpu_mpc_set_hessian_mode(qrgpu_ctx *ctx, int mode);

/* ---- batched device-pointer API (the measured path) -------------------------- */
/* d_type_id may be NULL (all robots type 0).  d_q: joint angles [12][n] (needed by the
 * J^T f torque map; pass fb_state + 13*n to reuse the WBC state).  d_status may be NULL. */
int qrgpu_mpc_solve_batch(qrgpu_ctx *ctx, int n, const int *d_type_id, const float *d_mpc_state,
                          const float *d_traj, const float *d_gait, const float *d_q,
                          float *d_force, float *d_tau_mpc, int *d_status);
int qrgpu_wbc_run_batch(qrgpu_ctx *ctx, int n, const int *d_type_id, const float *d_fb_state,
                        const float *d_wbc_cmd, float *d_prev_ori, float *d_tau,
                        float *d_qdes /* [24][n]: desiredJPos, desiredJVel; may be NULL */, int *d_status);
/* Full tick: MPC, then WBC with Fr_des := that MPC's forces (the Fr_des rows of d_wbc_cmd are ignored).
 * d_tau receives the WBC torque on stance legs and the MPC J^T f torque on swing legs
 * (UpdateLegCMD only overwrites stance legs, qr_wbc_locomotion_controller.cpp:205-219).
 * d_qdes [24][n] (may be NULL): desiredJPos, desiredJVel of the kinematic multitask projection (K12, qrMultitaskProjection::FindConfiguration,
 * which qrWbcLocomotionController::Run always executes, qr_wbc_locomotion_controller.cpp:124-129); with NULL that projection is skipped
 * (its outputs do not enter the torque). */
int qrgpu_tick_batch(qrgpu_ctx *ctx, int n, const int *d_type_id, const float *d_mpc_state,
                     const float *d_traj, const float *d_gait, const float *d_fb_state,
                     const float *d_wbc_cmd, float *d_prev_ori, float *d_force, float *d_tau, float *d_qdes, int *d_status);
/* The tick on the reference's cadence: per robot EITHER the MPC OR the WBC (wbcData.allowAfterMPC; qr_mpc_stance_leg_controller.cpp:337-382,
 * :129-156, :305-333; qr_fsm_state_locomotion.cpp:130-158), chosen by a device mask -- d_mpc_updated [n], the array qrgpu_mpc_frontend_batch
 * writes; any non-zero word means the robot is due.  d_force [12][n] and d_hold [12][n] are MEMORY: the caller's, required, carried from call to
 * call.  d_force is the world-frame f of the robot's last solve (what qrgpu_tick_batch writes; the WBC's Fr_des on held ticks), d_hold the
 * base-frame f_ff = -R^T f with R taken at that solve.  NULL for d_mpc_updated, d_force or d_hold: QRGPU_ERR_BAD_ARG, nothing is launched.
 *   due robot:   the MPC solve as in qrgpu_mpc_solve_batch.  d_force and d_hold are rewritten; d_tau = J^T f_ff on all legs with the context's torque
 *                epilogue on every motor, as qrgpu_mpc_solve_batch applies it; d_status is the solve's word.  The WBC does not touch the robot: its
 *                d_prev_ori column and d_qdes rows stay as they were.
 *   held robot:  no solve: d_force, d_hold, the warm-start words and the cost word are untouched.  d_tau = J(q_now)^T d_hold on all legs, then the
 *                WBC as in qrgpu_tick_batch: Fr_des from d_force, stance legs overwritten, the epilogue after the merge; d_qdes (may be NULL) is
 *                written.  d_status is the WBC's bits over an MPC part of 0 with iteration count 0 -- that count is how a held tick reads; there
 *                is no status bit for it.
 * Always the serial form on the context's stream, whatever qrgpu_set_tick_pipeline and qrgpu_set_tick_overlap say; no wait, poll or gate of its
 * own, and nothing is read back to the host: which robots are due is known on the device alone (qrgpu_set_stage_reset gives every robot its own
 * clock).  qrgpu_tick_batch remains the tick of the pipelined and overlapped forms.
 *   idle robot:  under qrgpu_set_mode_route (below, "the mode per robot") a robot that is not on the MPC chain is neither: nothing of it is read or
 *                written by any launch of the call.  With nothing bound there is no such robot. */
int qrgpu_tick_cadence_batch(qrgpu_ctx *ctx, int n, const int *d_type_id, const int *d_mpc_updated,
                             const float *d_mpc_state, const float *d_traj, const float *d_gait, const float *d_fb_state,
                             const float *d_wbc_cmd, float *d_prev_ori, float *d_force, float *d_hold,
                             float *d_tau, float *d_qdes, int *d_status);

/* Motor-command tail of the locomotion state (K14), off by default -- the single-robot drop-in keeps the FSM doing it:
 *   QRGPU_EPILOGUE_HIP_COMP  the +-0.9 N m abad compensation of qrFSMStateLocomotion::Run (QS/fsm/qr_fsm_state_locomotion.cpp:141-151:
 *                            legs FR, RR -0.9, legs FL, RL +0.9, added to every leg's command BEFORE the WBC overwrites its stance legs,
 *                            so in the full tick it survives on swing legs only; in qrgpu_mpc_solve_batch on every leg)
 *   QRGPU_EPILOGUE_CLIP      the +-23 N m clip of qrSafetyChecker::CheckForceFeedForward (QS/fsm/qr_safety_checker.cpp:48-66)
 * Applies to d_tau of qrgpu_tick_batch and qrgpu_mpc_solve_batch. */
#define QRGPU_EPILOGUE_HIP_COMP 1
#define QRGPU_EPILOGUE_CLIP     2
int qrgpu_set_torque_epilogue(qrgpu_ctx *ctx, int flags);

/* MPC front-end of n robots for one control tick: MPCStanceLegController::SetupCommand + Run + UpdateMPC without the solve
 * (QS/controllers/mpc/qr_mpc_stance_leg_controller.cpp:158-204, 207-334, 337-382).  Writes the contact table d_gait every tick,
 * the reference trajectory d_traj only for robots that re-plan this tick (iterationCounter % (round(dt_mpc/dt_ctrl)/2) == 0
 * or < 50; d_mpc_updated[i] = 1, may be NULL), and rows 0-14 and 63-66 of d_wbc_cmd (may be NULL): pBody_des, vBody_des,
 * aBody_des = 0, pBody_RPY_des, vBody_Ori_des, contact_state.  The horizon is the one of qrgpu_mpc_setup.
 * Reference values: dt_ctrl 0.002, dt_mpc 0.06, num_horizon_l = max(2, int(fullCyclePeriod/0.4)) (:43-50).
 * The re-plan period is round(dt_mpc/dt_ctrl)/2 by integer division (25 -> 12).  round(dt_mpc/dt_ctrl) must lie in 2 .. 2^24: below 2 the
 * reference takes a remainder by zero, so the call returns QRGPU_ERR_BAD_ARG and launches nothing.
 * iterationCounter is row 7 of d_fe_state, a float row that callers initialise with floats.  A float cannot count past 2^24 (9.3 h at 2 ms),
 * so a counter that would reach 2^24 is stored as the smallest value >= 50 of its residue class modulo the period: the cadence, which
 * only asks for counter % period and counter < 50, goes on exactly as the reference's integer counter would.  A caller that initialises the
 * row gives it a whole number in 0 .. 2^24 (0 after a Reset); the kernel converts it to int, so NaN and values beyond the int range are
 * undefined. */
int qrgpu_mpc_frontend_batch(qrgpu_ctx *ctx, int n, int num_horizon_l, float dt_ctrl, float dt_mpc, const float *d_fe_in,
                             float *d_fe_state, float *d_traj, float *d_gait, float *d_wbc_cmd, int *d_mpc_updated);

/* Force-balance stance forces of n robots: contact forces in the base frame, force[3*leg+axis] (the 3x4 matrix ComputeContactForce
 * returns, column-major) and, when d_q and d_tau are given, the joint torques J^T f of MapContactForceToJointTorques. */
/* d_type_id [n] may be NULL: every robot is then of type 0 (QRGPU_ERR_NOT_SETUP if type 0 was not set up).  With d_type_id, a robot whose
 * id is outside the table or names a type that was never set up is computed with the first type that was, and carries QRGPU_ST_BAD_TYPE
 * (QRGPU_ERR_NOT_SETUP if no type was set up at all).  The same holds for qrgpu_vmc_force_world_batch. */
int qrgpu_vmc_setup(qrgpu_ctx *ctx, int type_id, const qrgpu_vmc_desc *desc);
int qrgpu_vmc_force_batch(qrgpu_ctx *ctx, int n, const int *d_type_id, const float *d_vmc_in, const float *d_q /*[12][n], may be NULL*/,
                          float *d_force, float *d_tau /*may be NULL*/, int *d_status /*may be NULL*/);
/* The world-frame overload of ComputeContactForce (qr_qp_torque_optimizer.cpp:304-398; what TorqueStanceLegController::GetAction calls when
 * user_parameters.yaml computeForceInWorldFrame is true, qr_torque_stance_leg_controller.cpp:490-498): the same QP with, in d_vmc_in,
 * Rcb := rotMat (base -> world, quaternionToRotationMatrix(quat)^T), gvec := (0, 0, 9.8), normal := (0, 0, 1) -- the tangents are then the
 * world x and y axes, as GetAction passes them -- and per-leg force-window ratios d_ratio [8][n] = fMinRatio[4], fMaxRatio[4] (the Vec4
 * members that the walk mode changes per tick, :128-152).  Forces come back in the base frame, as RigidTransform(0, quat, X^T) returns them.
 * d_type_id may be NULL (type 0), as above.  The reference runs this overload with frictionCoef = 0.6 (see qrgpu_vmc_desc). */
int qrgpu_vmc_force_world_batch(qrgpu_ctx *ctx, int n, const int *d_type_id, const float *d_vmc_in, const float *d_ratio, const float *d_q,
                                float *d_force, float *d_tau, int *d_status);

/* Base velocity estimator (TinyEKF<3,3> + moving-window filters), the leg kinematics it reads and the pose estimator that follows it
 * (stance-foot height, planar odometry), for n robots and one control tick.
 * d_est_state is the estimators' memory: qrgpu_estimator_state_doubles(window) doubles per robot, [field][robot], zero = freshly
 * constructed / Reset() (qr_robot_velocity_estimator.cpp:29-60).  d_tick: robot->GetTick() in milliseconds.  All robots share `desc`. */
typedef struct {
    float hip_l, upper_l, lower_l;
    float hip_offset[12];                 /* GetDefaultHipPosition, 3*leg+axis */
    float time_step;                      /* robot->timeStep, used for the first sample */
    float accelerometer_variance, sensor_variance;   /* user_parameters.yaml: 0.1, 0.1 */
    int window;                           /* movingWindowFilterSize: 120 */
    float body_height;                    /* robot->bodyHeight, the height reported while no foot is in stance */
} qrgpu_estimator_desc;
void qrgpu_estimator_desc_default(qrgpu_estimator_desc *d);
int qrgpu_estimator_state_doubles(int window);
#define QRGPU_EST_IN_ROWS  54     /* rows of est_in  */
#define QRGPU_EST_OUT_ROWS 42     /* rows of est_out */
int qrgpu_estimator_update_batch(qrgpu_ctx *ctx, int n, const qrgpu_estimator_desc *desc, const float *d_est_in, const unsigned *d_tick,
                                 double *d_est_state, float *d_est_out);

/* Ground-plane fit and control frame of n robots for one control tick: qrGroundSurfaceEstimator::Update / GetNormalVector /
 * ComputeControlFrame (QS/estimators/qr_ground_surface_estimator.cpp:40-70,151-206), which qrStateEstimatorContainer::Update runs in front
 * of the robot estimator (QI/estimators/qr_state_estimator_container.h:76-81).  The fit fires when all four feet are in contact and one of
 * them newly so; the control frame is the base's heading (the reference assumes a flat ground in the world, :168), low-pass filtered as
 * roll / pitch / yaw with ratio 0.8 and roll := 0.
 * d_ground_in [23][n]: footContact[4], footPositionsInBaseFrame[12] (3*leg+axis), basePosition[3], quat_wxyz[4].
 * d_ground_state [QRGPU_GROUND_STATE_DOUBLES][n] doubles is the estimators' memory (lastContactState[4], a[3], n[3], controlFrameRPY[3]);
 * reset != 0 applies Reset() before the update.  d_ground_out [QRGPU_GROUND_OUT_ROWS][n] (may be NULL): plane coefficients a[3]
 * (z = a0 + a1 x + a2 y, base frame), unit normal n[3], controlFrameRPY[3], controlFrameOrientation[4], stateDataFlow.groundRMat[9]
 * (row-major), stateDataFlow.baseRInControlFrame[9], updated flag.  d_est_in (may be NULL): the estimator's input array, whose rows 45-53
 * (GetAlignedDirections) receive groundRMat, so that ground fit -> pose estimator stays on the device. */
#define QRGPU_GROUND_IN_ROWS 23
#define QRGPU_GROUND_STATE_DOUBLES 13
#define QRGPU_GROUND_OUT_ROWS 32
int qrgpu_ground_update_batch(qrgpu_ctx *ctx, int n, int reset, const float *d_ground_in, double *d_ground_state, float *d_ground_out,
                              float *d_est_in);

/* Open-loop gait generator (qrOpenLoopGaitGenerator::Update + Schedule, QS/gait/qr_openloop_gait_generator.cpp:126-249) of n robots for
 * one control tick.  d_contact [4][n]: robot->GetFootContact().  d_gait_state [QRGPU_GAIT_STATE_FLOATS][n] is the generators' memory;
 * reset: 0 = carry on; QRGPU_GAIT_RESET_CONSTRUCT (1) = a generator as constructed followed by Reset(0): the state array's earlier content is not
 * read (the first call on a state array); QRGPU_GAIT_RESET_LIVE (2) = Reset(0) on the RUNNING generator before the update, which in the reference
 * (QI/gait/qr_gait.h:76-87) rewrites resetTime, lastTime, normalizedPhase, the four leg-state vectors and contactStartPhase and leaves gaitCycle,
 * cumDt, firstSwing, firstStance, swingTimeRemaining and phaseInFullCycle as they were -- it READS the state array, so it must never be the
 * first call on one.  NOTE: the numbers are the other way round from qrgpu_walk_gait_update_batch and qrgpu_swing_update_batch (2 = as
 * constructed, 1 = Reset()): 1 keeps the meaning this entry point's "reset != 0" always had; use the names.  Any other value: QRGPU_ERR_BAD_ARG.
 * d_gait_out [24][n] (may be NULL): phaseInFullCycle[4], normalizedPhase[4],
 * desiredLegState[4], legState[4], curLegState[4], swingTimeRemaining[4].  d_fe_in (may be NULL): the front-end's input array, whose rows
 * 42-61 (phaseInFullCycle, dutyFactor, normalizedPhase, desiredLegState, legState) are written.  Legs with duty factor 0
 * (USERDEFINED_SWING) are not supported. */
#define QRGPU_GAIT_STATE_FLOATS 52
#define QRGPU_GAIT_RESET_CONSTRUCT 1
#define QRGPU_GAIT_RESET_LIVE 2
typedef struct {
    float stance_duration[4], duty_factor[4], initial_leg_phase[4];   /* openloop_gait_generator.yaml: 0.5, 0.6, (0.5, 0, 0, 0.5) for advanced_trot */
    int initial_leg_state[4];                                          /* LegState: SWING 0, STANCE 1 */
    float contact_detection_phase_threshold, wait_time;                /* 0.5, gait_params.wait_time */
    int advanced_trot;                                                 /* gait == "advanced_trot": the lost-contact hold of Schedule() */
} qrgpu_gait_desc;
void qrgpu_gait_desc_default(qrgpu_gait_desc *d);
int qrgpu_gait_update_batch(qrgpu_ctx *ctx, int n, const qrgpu_gait_desc *desc, float current_time, int robot_stop, int reset, const float *d_contact,
                            float *d_gait_state, float *d_gait_out, float *d_fe_in);

/* Walk gait generator of n robots for one control tick (qrWalkGaitGenerator::Update, QS/gait/qr_walk_gait_generator.cpp:202-288; the
 * constructor's bookkeeping :66-193 is done on the host from `desc`), and the contacts / force-window ratios its sub-states select in
 * TorqueStanceLegController::UpdateFRatio's walk branch (QS/controllers/balance_controller/qr_torque_stance_leg_controller.cpp:125-168).
 * current_time is the time the reference passes to Update (it is NOT taken relative to the last reset there).  d_contact [4][n]:
 * robot->GetFootContact().  d_walk_state [QRGPU_WALK_STATE_FLOATS][n] is the generators' memory; reset: 2 = as constructed, 1 = Reset()
 * (stateIndexOfLegs and the detection members survive a Reset in the reference), 0 = carry on.
 * d_walk_out [QRGPU_WALK_OUT_ROWS][n] (may be NULL): phaseInFullCycle[4], normalizedPhase[4], desiredLegState[4] (LegState /
 * SubLegState values: STANCE 1, LOAD_FORCE 5, UNLOAD_FORCE 6, FULL_STANCE 7, TRUE_SWING 8), legState[4], curLegState[4],
 * detectedLegState[4] (SWING 0, STANCE 1, EARLY_CONTACT 2, LOSE_CONTACT 3), detectedEventTickPhase[4], moveBasePhase, contacts[4],
 * fMinRatio[4], fMaxRatio[4].  d_ratio [8][n] (may be NULL): fMinRatio, fMaxRatio laid out as qrgpu_vmc_force_world_batch takes them;
 * d_vmc_in (may be NULL): its rows 18-21 (contacts) are written.  Legs with duty factor 0 (USERDEFINED_SWING) are not supported; members the
 * reference leaves uninitialised until their first write (moveBasePhase, detectedLegState, detectedEventTickPhase) start at zero. */
#define QRGPU_WALK_STATE_FLOATS 33
#define QRGPU_WALK_OUT_ROWS 41
typedef struct {
    float stance_duration[4], duty_factor[4], initial_leg_phase[4];   /* openloop_gait_generator.yaml, gait "walk": 7.5, 0.75, (0.5, 0, 0.75, 0.25) */
    int initial_leg_state[4];                                          /* LegState: SWING 0, STANCE 1 */
    float contact_detection_phase_threshold;                           /* 0.1 */
    int n_states;                                                      /* entries of state_switch_que / state_ratio (<= 4) */
    int state_switch[4];                                               /* SubLegState: full_stance 7, unload_force 6, true_swing 8, load_force 5 */
    float state_ratio[4];                                              /* 0.2, 0.3, 0.3, 0.2 */
} qrgpu_walk_gait_desc;
void qrgpu_walk_gait_desc_default(qrgpu_walk_gait_desc *d);
int qrgpu_walk_gait_update_batch(qrgpu_ctx *ctx, int n, const qrgpu_walk_gait_desc *desc, float current_time, int robot_stop, int reset,
                                 const float *d_contact, float *d_walk_state, float *d_walk_out, float *d_ratio, float *d_vmc_in);

/* Swing-leg targets of the MPC/WBC mode (qrRaibertSwingLegController::GetAction, ADVANCED_TROT case on horizontal terrain,
 * QS/controllers/qr_swing_leg_controller.cpp:362-398,408-424): XY-linear / Z-parabola foot trajectory between the lift-off point and the
 * planned foothold, its world-frame image for the WBC foot tasks, and the inverse-kinematics joint targets of the swing command.
 * swing_in [58][n]: swing flag[4], footholdPlanner phase[4], swingDuration[4], phaseSwitchFootGlobalPos[12], desiredFootholds[12] (base
 * frame), basePosition[3], quat_wxyz[4], baseVInWorldFrame[3], motor angles[12].  For the flagged legs only: rows 15-50 of d_wbc_cmd
 * (pFoot_des, vFoot_des, aFoot_des), d_foot_target_world [12][n] (footTargetPositionsInWorldFrame, rows 26-37 of fe_in) and
 * d_qdes [24][n] (joint angle and velocity targets).  Any output may be NULL.  desc: leg lengths and hip offsets. */
int qrgpu_swing_targets_batch(qrgpu_ctx *ctx, int n, const qrgpu_estimator_desc *desc, const float *d_swing_in, float *d_wbc_cmd,
                              float *d_foot_target_world, float *d_qdes);

/* Swing-leg action of the velocity mode -- the trot that the force-balance path (qrgpu_vmc_force_batch) belongs to:
 * qrRaibertSwingLegController::GetAction, VELOCITY_LOCOMOTION case (QS/controllers/qr_swing_leg_controller.cpp:285-309, 408-424): the
 * Raibert target in the base frame from the hip's horizontal velocity, XYLinear_ZParabola (height 0.1) between the lift-off point and that
 * target at the warped phase of GenerateTrajectoryPoint(phaseModule = true), leg inverse kinematics.
 * swing_vel_in [53][n]: swing flag[4] (the leg is in swingFootIds), normalizedPhase[4], phaseSwitchFootLocalPos[12] (3*leg+axis), estimated
 * base velocity in the base frame[3], yaw rate, desiredSpeed[3] (stateDes 6..8), desiredTwistingSpeed (stateDes 11), dR[9]
 * (stateDataFlow.baseRInControlFrame, row-major: rows 22-30 of qrgpu_ground_update_batch's output; the identity on PLANE / PLUM_PILES
 * terrain), quat_wxyz[4], motor angles[12].  d_out [48][n], for the flagged legs only: footTargetPosition[12] (base frame),
 * footPositionInBaseFrame[12], joint angle targets[12], joint velocity targets[12] (zero: the reference's parabola generator returns no
 * velocity).  desc: leg lengths and robot->hipOffset (the inverse kinematics); vdesc: the controller's own parameters. */
typedef struct {
    float hip_position_com[12];       /* GetDefaultHipPosition() + comOffset, 3*leg+axis                              */
    float stance_duration[4];         /* gaitGenerator->stanceDuration                                                */
    float swing_kp[3];                /* user_parameters.yaml swingKp.trot: 0.03 x3                                   */
    float desired_height;             /* user_parameters desiredHeight - footClearance: 0.26                          */
} qrgpu_swing_velocity_desc;
int qrgpu_swing_velocity_batch(qrgpu_ctx *ctx, int n, const qrgpu_estimator_desc *desc, const qrgpu_swing_velocity_desc *vdesc,
                               const float *d_swing_vel_in, float *d_out);

/* Swing-leg selection and the Raibert-type foothold heuristic that feed qrgpu_swing_targets_batch: qrRaibertSwingLegController::Update
 * (default branch, QS/controllers/qr_swing_leg_controller.cpp:211-236) + qrFootholdPlanner::ComputeHeuristicFootHold
 * (QS/planner/qr_foothold_planner.cpp:110-239) on flat ground (groundRMat = I).
 * fh_in [46][n]: legState[4] (LegState: SWING 0, STANCE 1, EARLY_CONTACT 2, LOSE_CONTACT 3), allowSwitchLegState[4], swingTimeRemaining[4],
 * normalizedPhase[4], desiredSpeed[3] (stateDes 6..8), desiredTwistingSpeed (stateDes 11), stateDes(2), footPositionsInBaseFrame[12],
 * quat_wxyz[4], rpy[3], baseVelocityInBaseFrame[3], baseRollPitchYawRate[3].  When d_gait_state / d_gait_out (the arrays of
 * qrgpu_gait_update_batch) are given, rows 0-15 are taken from them instead.  Writes swing_in rows 0-3 (leg is in swingFootIds) for every
 * leg and, for those legs, rows 4-7 (footholdPlanner->phase) and 24-35 (desiredFootholds, base frame); other rows are left alone.
 * The reference's out-of-bounds write for backwards commands (:222-225, footTargetPosition(0,2) on a 3x1 vector) is not reproduced. */
typedef struct {
    float hip_offset[12];             /* robot->hipOffset, 3*leg+axis (robot_params.hip_offset)                      */
    float default_hip_position[12];   /* robot->GetDefaultHipPosition() (robot_params.default_hip_positions)         */
    float hip_l;                      /* robot->hipLength                                                             */
    float swing_kp[3];                /* user_parameters.yaml swingKp.advanced_trot: 0.16 x3                          */
    float foot_clearance;             /* user_parameters.yaml footClearance: 0.01                                     */
} qrgpu_foothold_desc;
void qrgpu_foothold_desc_default(qrgpu_foothold_desc *d);
int qrgpu_footholds_batch(qrgpu_ctx *ctx, int n, const qrgpu_foothold_desc *desc, const float *d_fh_in, const float *d_gait_state,
                          const float *d_gait_out, float *d_swing_in);

/* Swing-leg controller of the walk and position modes, and the lift-off memory of all four modes (qrRaibertSwingLegController::Reset /
 * Update / GetAction, QS/controllers/qr_swing_leg_controller.cpp:60-101,104-229,241-461, with qrFootholdPlanner::Reset / UpdateOnce,
 * QS/planner/qr_foothold_planner.cpp:49-109, and qrFootStepper's gap-crossing plan, QS/planner/qr_foot_stepper.cpp:31-202,483-525).
 * Modes are LocomotionMode: VELOCITY 0, POSITION 1, WALK 2, ADVANCED_TROT 3; terrains TerrainType: PLANE 0, PLUM_PILES 1, STAIRS 2,
 * SLOPE 3, ROUGH 4 (config/qr_enum_types.h:62-92).
 * Inputs are the arrays the device already holds: est_in (quat_wxyz rows 6-9, motor angles 17-28), est_out (footPositionsInBaseFrame
 * rows 12-23, basePosition 36-38) and the gait generator's output: for WALK the [QRGPU_WALK_OUT_ROWS][n] output of
 * qrgpu_walk_gait_update_batch, for the other modes the [24][n] output of qrgpu_gait_update_batch with its [QRGPU_GAIT_STATE_FLOATS][n]
 * state (allowSwitchLegState; read by the position mode's action only).  Both outputs keep desiredLegState in rows 8-11, legState in
 * 12-15, curLegState in 16-19 and normalizedPhase in 4-7; the walk output's detectedLegState is rows 20-23.
 * d_swing_state [QRGPU_SWING_STATE_FLOATS][n] is the controller's memory:
 *   0-11  phaseSwitchFootLocalPos (3*leg+axis)        12-23 phaseSwitchFootGlobalPos      24-35 footHoldInWorldFrame
 *   36-47 walk trajectory source                      48-59 walk trajectory target        60-63 walk trajectory height (stepParams.height)
 *   64    walk trajectory built, bit per leg          65-76 last joint angle targets      77-88 last joint velocity targets
 *   89    swingJointAnglesVelocities entry, bit per leg                                   90-101 desiredFootholdsOffset (3*leg+axis)
 *   102   stepper flags: 1 generatorFlag, 2 gaitFlag  103 / 104 plan queue head / tail    105-... plan queue, 4 floats per step
 * d_swing_flags: one word per robot of QRGPU_SW_* bits (not the tick's status word), cleared by a reset, OR-ed by both calls: the cases in
 * which the reference is undefined or ends the process.  The plan keeps the steps made before QRGPU_SW_PLAN_EXIT / _FULL; a -1 shift on an
 * empty plan shifts the planning position only.
 * Deliberate readings: the unqualified abs on floats (qr_foot_trajectory_generator.cpp:100,105,123,298, qr_foot_stepper.cpp:150) is
 * std::abs(float); CheckSolution's QP is QuadProg++'s Goldfarb-Idnani iteration for one variable, step for step; MAXIMUM_STEP = 0.001
 * (config/qr_config.h:43) is kept, so every step that meets a gap returns -1 or -2 as in the reference. */
#define QRGPU_MODE_VELOCITY 0
#define QRGPU_MODE_POSITION 1
#define QRGPU_MODE_WALK 2
#define QRGPU_MODE_ADVANCED_TROT 3
#define QRGPU_SWING_MAX_GAPS 8
#define QRGPU_SWING_MAX_PLAN 32
#define QRGPU_SWING_STATE_FLOATS (105 + 4 * QRGPU_SWING_MAX_PLAN)
#define QRGPU_SWING_OUT_ROWS 52
#define QRGPU_SW_NO_TRAJECTORY 0x1   /* a WALK leg swings before a lift-off built its trajectory (the reference reads an unset generator) */
#define QRGPU_SW_PHASE_RANGE   0x2   /* a WALK phase outside [-1e-3, 1 + 1e-3): GenerateTrajectory fails and GetAction throws (:352-354) */
#define QRGPU_SW_PLAN_EXIT     0x4   /* StepGenerator returned -2: exit(-1) in GetOptimalFootholdsOffset (:501-503) */
#define QRGPU_SW_PLAN_EMPTY    0x8   /* a -1 cross-gait shift before any step was planned: steps.back() on an empty queue (:505-507) */
#define QRGPU_SW_PLAN_FULL     0x10  /* the plan needs more than QRGPU_SWING_MAX_PLAN steps */
typedef struct {
    int   mode, terrain, is_sim;      /* controlParams["mode"]; TerrainType after the ground estimator's Reset
                                         (qr_ground_surface_estimator.cpp:73-100: POSITION forces PLUM_PILES); robot->isSim */
    float foothold_delta;             /* qrFootStepper defaultFootholdDelta: 0.10 (qr_foothold_planner.cpp:44) */
    int   n_gaps;                     /* terrain.yaml gaps, read on PLUM_PILES only (a1_sim: 0.51, 1.31, 1.91, gap_width 0.14) */
    float gap_distance[QRGPU_SWING_MAX_GAPS], gap_width;
} qrgpu_swing_mode_desc;
/* mode's defaults for config/a1_sim: POSITION on PLUM_PILES with a1_sim's gaps, WALK on SLOPE (terrain.yaml), VELOCITY on SLOPE,
 * ADVANCED_TROT on STAIRS; is_sim 1 */
void qrgpu_swing_mode_desc_default(qrgpu_swing_mode_desc *d, int mode);
/* Reset (reset: 2 = as constructed, 1 = Reset(), which keeps the stepper's plan and flags and the walk trajectories, 0 = carry on) and
 * Update for one control tick.  The first call on a state array must use reset = 2 (the plan queue's head and tail are clamped to the
 * array, so an uninitialised one gives wrong footholds, not a wrong address).  Lift-off triggers: POSITION SWING / USERDEFINED_SWING from STANCE, WALK TRUE_SWING / USERDEFINED_SWING
 * from UNLOAD_FORCE (both not while robot_stop), VELOCITY / ADVANCED_TROT a change to SWING.  POSITION plans the footholds of all legs at
 * leg 0's lift-off (the gap plan is made once per constructed controller), WALK builds the leg's B-spline (source and target in the world
 * frame when is_sim, else in the base frame).  For VELOCITY and ADVANCED_TROT, when given, the rows the existing kernels read receive the
 * lift-off point at every reset and lift-off: d_swing_in rows 12-23 (phaseSwitchFootGlobalPos = baseRMat * local, no translation, as
 * :186 has it), d_swing_vel_in rows 8-19 (phaseSwitchFootLocalPos) and d_fe_in rows 62-63 (firstSwingBaseState x, y: at a reset, and at
 * ADVANCED_TROT lift-offs); other rows are left alone.  d_gait_state is not read (may be NULL). */
int qrgpu_swing_update_batch(qrgpu_ctx *ctx, int n, const qrgpu_swing_mode_desc *desc, int reset, int robot_stop, const float *d_est_in,
                             const float *d_est_out, const float *d_gait_out, const float *d_gait_state, float *d_swing_state,
                             float *d_swing_in, float *d_swing_vel_in, float *d_fe_in, int *d_swing_flags);
/* GetAction of the POSITION and WALK modes (VELOCITY and ADVANCED_TROT have qrgpu_swing_velocity_batch / qrgpu_swing_targets_batch):
 * swing-leg selection (:204-229), POSITION's XY-linear / Z-parabola between the world lift-off point and footHoldInWorldFrame at the
 * warped phase, WALK's B-spline at normalizedPhase (velocity per unit phase, as the reference's), the frame change RigidTransform, leg IK
 * and J^-1 v (a NaN angle keeps the current one), and the command loop over the swingJointAnglesVelocities entries (:427-459).
 * d_out [QRGPU_SWING_OUT_ROWS][n]: foot position in the base frame[12], foot velocity in the base frame[12], joint angle targets[12],
 * joint velocity targets[12] (3*leg+axis), command flags[4].  The flags are written for every leg; the other rows for the legs this call
 * computed (rows 0-47) or commands (rows 24-47: an entry of an earlier swing re-emits its last targets).  geom: leg lengths and hip offsets. */
int qrgpu_swing_action_batch(qrgpu_ctx *ctx, int n, const qrgpu_swing_mode_desc *desc, const qrgpu_estimator_desc *geom, int robot_stop,
                             const float *d_est_in, const float *d_est_out, const float *d_gait_out, const float *d_gait_state,
                             float *d_swing_state, float *d_out, int *d_swing_flags);

/* Stance front-end and motor commands of the force-balance modes (VELOCITY, POSITION, WALK, ADVANCED_TROT without MPC):
 * TorqueStanceLegController::UpdateFRatio / UpdateDesCommand / GetAction's command tail (QS/controllers/balance_controller/
 * qr_torque_stance_leg_controller.cpp:89-172, 174-477, 503-541) and qrLocomotionController::GetAction's merge (qr_locomotion_controller.cpp:
 * 128-147).  With these a force-balance tick is queued entirely on the context's stream: ground, estimator, gait, swing update, stance
 * tick, swing action -- no host copy in between.
 * qrgpu_stance_update_batch reads arrays the device already holds:
 *   d_est_in     quat_wxyz rows 6-9, rpyRate 10-12 (the tick also takes the motor angles, rows 17-28, for the J^T f torque map)
 *   d_est_out    baseVelocityInBaseFrame 6-8, footPositionsInBaseFrame 12-23, basePosition 36-38, heightInControlFrame 39
 *   d_ground_out controlFrameRPY 6-8, controlFrameOrientation 9-12, groundRMat 13-21, baseRInControlFrame 22-30
 *   d_rpy [3][n] GetBaseRollPitchYaw, as qrgpu_pack_state_batch takes it
 *   d_gait_out   WALK: the [QRGPU_WALK_OUT_ROWS][n] output of qrgpu_walk_gait_update_batch (normalizedPhase 4-7, desiredLegState 8-11,
 *                detectedLegState 20-23, moveBasePhase 28, contacts 29-32, fMinRatio 33-36, fMaxRatio 37-40: the walk branch of UpdateFRatio
 *                is computed there); other modes: the [24][n] output of qrgpu_gait_update_batch (normalizedPhase 4-7, desiredLegState 8-11,
 *                legState 12-15)
 *   d_gait_state the open-loop generator's state (allowSwitchLegState, rows 20-23): needed by POSITION and ADVANCED_TROT, else may be NULL
 *   d_stance_cmd [QRGPU_STANCE_CMD_ROWS][n], the one input that comes from the host, and changes only when the operator's command or the walk
 *                pose plan does: row 0 stateDes(2); 1-3 stateDes 6..8; 4-6 stateDes 9..11; 7-12 the pose planner's segment source (the pose at
 *                its last Update / ResetBasePose); 13-18 poseDest; 19-24 twist (rows 7-24 are what qrgpu_pose_plan_batch writes on the device);
 *                25-27 footholdPlanner->GetDesiredComPose().tail(3)
 *   d_stance_state [QRGPU_STANCE_STATE_FLOATS][n] the controller's memory: row 0 heightInControlFrame, which est_out reports as NaN while no
 *                foot is in stance and the reference then keeps; reset != 0 starts it at desc->body_height (qr_robot_pose_estimator.cpp:50)
 * current_time and desc->pose_reset_time give the WALK pose phase while robot_stop (GetIntermediateBasePose(currentTime)); otherwise that
 * phase is moveBasePhase.  Under a stage-reset binding with d_ticks (qrgpu_set_stage_reset) current_time is the robot's own;
 * desc->pose_reset_time stays one scalar for the batch (it is read only while robot_stop; a per-robot pose-planner reset time is out of scope).
 * robot_stop (:95-102) sets every contact, ratios 0.01 / 10 and N = 4 in every mode, over what the walk kernel wrote.
 * In POSITION mode qrComAdjuster::Update runs in the kernel (erf in double); in ADVANCED_TROT the reference never calls it, so
 * comPosInBaseFrame is the zero vector of its Reset.  Dead branches of the reference that are not built: qr_stance_kernel.hip's header.
 * Outputs, each may be NULL:
 *   d_vmc_in [37][n] complete: foot positions, desiredAcc, contacts and Rcb / g / surfaceNormal as the overload the mode selects builds
 *                them -- control frame (qr_qp_torque_optimizer.cpp:202-221): identity, (0, 0, 9.8), e_z on PLANE / PLUM_PILES, else
 *                groundRMat^T baseRMat, groundRMat^T g, (-sin pitch, 0, cos pitch); world frame (:319-336): baseRMat, (0, 0, 9.8), e_z
 *   d_ratio [8][n]  fMinRatio[4], fMaxRatio[4]
 *   d_stance_out [QRGPU_STANCE_OUT_ROWS][n]: stateCur[12], stateDes[12], ddqDes[6], N (row 30), moveBasePhase (31), computeForceInWorldFrame
 *                (32: 1 = the tick needs qrgpu_vmc_force_world_batch; WALK always, ADVANCED_TROT with desc->force_in_world)
 * qrgpu_stance_command_batch writes d_motor_cmd [QRGPU_MOTOR_CMD_ROWS][n] = p[12], Kp[12], d[12], Kd[12], tua[12] (qrMotorCommand, motor-major
 * inside each field) from d_tau [12][n] (the QP's J^T f): {0, 0, 0, 0, tau}; in WALK {0, 0.0 kp, 0, 0.5 kd, tau} for a leg in contact (rows 18-21
 * of d_vmc_in; the reference's 0.0 * legJointq is written as 0), {0, 0, 0, 0.0 kd, tau} when (N < 4 && moveBasePhase < 0.7) || robot_stop
 * (rows 30, 31 of d_stance_out), else all zero.  d_swing_q [24][n] (joint angle and velocity targets) and d_swing_flag [4][n] -- rows 24-47
 * and 48-51 of qrgpu_swing_action_batch's output for POSITION / WALK, the caller's own arrays otherwise; both NULL: no swing command --
 * make a flagged leg's motors {q, kp, qd, kd, 0} (qr_swing_leg_controller.cpp:456-458).  d_vmc_in / d_stance_out are read in WALK only.
 * qrgpu_stance_tick_batch: update, the QP overload the mode selects (d_type_id as in the VMC calls; joint angles from d_est_in), command:
 * three launches on the context's stream, results those of the three calls made one by one, bit for bit.  It needs d_vmc_in, d_force,
 * d_tau, d_motor_cmd, d_ratio for the world-frame overload and d_stance_out in WALK.
 * QRGPU_ERR_BAD_ARG (outputs untouched): a mode or terrain outside the enums, a NULL required array, n < 1 or n > max_batch. */
#define QRGPU_STANCE_CMD_ROWS 28
#define QRGPU_STANCE_STATE_FLOATS 1
#define QRGPU_STANCE_OUT_ROWS 33
#define QRGPU_MOTOR_CMD_ROWS 60
typedef struct {
    int   mode, terrain;              /* LocomotionMode, TerrainType (as qrgpu_swing_mode_desc) */
    int   force_in_world;             /* user_parameters.yaml computeForceInWorldFrame; read by ADVANCED_TROT only (VELOCITY and POSITION
                                         clear it, WALK sets it) */
    float kp[6], kd[6], max_ddq[6], min_ddq[6];   /* stance_leg_controller.yaml stance_leg_params of the mode */
    float desired_height, desired_speed[3], desired_twisting_speed;   /* user_parameters.yaml: 0.27, (0, 0, 0), 0 */
    float body_height;                /* robot->bodyHeight: 0.28 */
    float pose_reset_time;            /* qrPosePlanner::resetTime (ResetBasePose) */
    float motor_kp[12], motor_kd[12]; /* robot->GetMotorKps / GetMotorKdp: (100, 100, 100) / (1, 2, 2) per leg */
} qrgpu_stance_desc;
/* config/a1_sim for the mode; terrain as qrgpu_swing_mode_desc_default, force_in_world 1 (user_parameters.yaml:40) */
void qrgpu_stance_desc_default(qrgpu_stance_desc *d, int mode);
int qrgpu_stance_update_batch(qrgpu_ctx *ctx, int n, const qrgpu_stance_desc *desc, float current_time, int robot_stop, int reset,
                              const float *d_est_in, const float *d_est_out, const float *d_ground_out, const float *d_rpy, const float *d_gait_out,
                              const float *d_gait_state, const float *d_stance_cmd, float *d_stance_state, float *d_vmc_in, float *d_ratio,
                              float *d_stance_out);
int qrgpu_stance_command_batch(qrgpu_ctx *ctx, int n, const qrgpu_stance_desc *desc, int robot_stop, const float *d_vmc_in,
                               const float *d_stance_out, const float *d_tau, const float *d_swing_q, const float *d_swing_flag, float *d_motor_cmd);
int qrgpu_stance_tick_batch(qrgpu_ctx *ctx, int n, const qrgpu_stance_desc *desc, float current_time, int robot_stop, int reset,
                            const int *d_type_id, const float *d_est_in, const float *d_est_out, const float *d_ground_out, const float *d_rpy,
                            const float *d_gait_out, const float *d_gait_state, const float *d_stance_cmd, float *d_stance_state, float *d_vmc_in,
                            float *d_ratio, float *d_stance_out, float *d_force, float *d_tau, int *d_status, const float *d_swing_q,
                            const float *d_swing_flag, float *d_motor_cmd);

/* Walk pose planner: qrPosePlanner::Update with its SQP (QS/planner/qr_pose_planner.cpp:72-456: 20 iterations, each a 6-variable QuadProg++
 * solve with 3N = 9 or 12 inequality rows) and ResetBasePose (QI/planner/qr_pose_planner.h:311-320), one wavefront per robot.  It writes the
 * rows of d_stance_cmd that qrgpu_stance_update_batch reads in WALK, so a WALK tick is queued on the context's stream with no host copy:
 * ground, estimator, walk gait, pose plan, swing update, stance tick, swing action.
 * Inputs, the arrays and rows of qrgpu_stance_update_batch: d_est_in quat_wxyz 6-9 (GetBaseOrientation); d_est_out
 * footPositionsInBaseFrame 12-23, basePosition 36-38; d_ground_out controlFrameRPY 6-8 (row 7, the pitch, is the one value the planner uses;
 * controlFrameOrientation 9-12 only enters values the reference computes and never reads); d_rpy [3][n] GetBaseRollPitchYaw; d_walk_out
 * desiredLegState 8-11, legState 12-15, curLegState 16-19.  Foot positions in the world frame are invertRigidTransform(basePosition, quat,
 * footPositionsInBaseFrame) (qr_robot.cpp:222-230).  GetEstimatedPosition() is taken from d_est_out rows 36-38, as the stance kernel takes
 * the base position: in the reference qrRobotEstimator::estimatedPosition is its own member, filled from the pose estimator's pose
 * (qr_robot_estimator.cpp:40,58,87), which is also what robot->basePosition receives; this ABI has one array for both.
 * event, with d_event NULL, applies to every robot: 0 nothing (with reset == 0 the call returns without a launch), 1 Update, 2 ResetBasePose,
 * 3 Update for exactly the robots with a leg whose legState is SWING (0) and curLegState STANCE (1) -- the switchToSwing rule of
 * qr_locomotion_controller.cpp:81-89 (USERDEFINED_SWING legs are not built in this library's walk gait).  d_event [n] non-NULL: its values
 * 0 / 1 / 2 per robot win (anything else is 0).  The swing semaphore and robot->stop stay with the caller.
 * reset != 0 first puts every robot's d_pose_state into the constructed state (:31-69): Lambda 0.1 x 12, size 12, quat identity, rIB the
 * estimated position, poseDest (rIB, 0, 0, 0).
 * d_pose_state [QRGPU_POSE_STATE_ROWS][n], the members the reference keeps between calls or publishes: rows 0-11 Lambda, 12 its current
 * size (3N of the last Update; conservativeResize(3N) truncates it), 13-15 rIB, 16-19 quat, 20-25 poseDest.  Lambda(i) = u[i] of the last
 * QP, u indexed by working-set SLOT as solve_quadprog_test returns it, not by constraint.
 * d_stance_cmd [QRGPU_STANCE_CMD_ROWS][n]: for a robot with an event and no fatal flag rows 7-12 (segment source: estimated position,
 * d_rpy), 13-18 (poseDest) and, ResetBasePose only, 19-24 (twist = 0) are written; every other row and robot is left as it was.
 * d_pose_out [QRGPU_POSE_OUT_ROWS][n] (may be NULL; inspection, Update only): rows 7k .. 7k+5 the step p of SQP iteration k and 7k+6 the
 * size of the working set its QP ended with (iterations >= loops are not written); 140-151 the final Lambda (0 beyond 3N); 152 N;
 * 153 the vertices kept, bit per counter-clockwise slot (slot c is leg {0, 2, 3, 1}[c]); 154-165 u of iteration 0 (0 beyond 3N);
 * 166-177 the working set A[] of iteration 0 in slot order (-1 beyond its size).
 * d_pose_flags [n] (required): QRGPU_PP_* bits of the robot's last event, written for every robot with an event.  FEW_CONTACTS, NOT_PD and
 * NAN are fatal: the robot's rows of d_stance_cmd and d_pose_state stay untouched.
 * desc->rBH is 3*leg+axis in leg order; desc->loops is clamped to 1 .. QRGPU_POSE_MAX_LOOPS.
 * QRGPU_ERR_BAD_ARG (outputs untouched): a NULL required array, n < 1 or n > max_batch, event outside 0..3. */
#define QRGPU_POSE_MAX_LOOPS  20
#define QRGPU_POSE_STATE_ROWS 26
#define QRGPU_POSE_OUT_ROWS   (7 * QRGPU_POSE_MAX_LOOPS + 38)
#define QRGPU_PP_FEW_CONTACTS 0x1    /* fewer than 3 valid vertices: the reference throws "N < 3" (with no contact it first divides by zero) */
#define QRGPU_PP_NOT_PD       0x2    /* QuadProg++'s Cholesky would throw: hessF - sum Lambda hessG is not positive definite */
#define QRGPU_PP_INFEASIBLE   0x4    /* a QP returned +inf with the iterate it had; the reference goes on with that x and u, so does the kernel */
#define QRGPU_PP_LAMBDA_GROWN 0x8    /* 3N exceeds Lambda's size: the reference reads uninitialised entries, the kernel uses 0.1 */
#define QRGPU_PP_NONCONVEX    0x10   /* the convexity test of :138-168 erased a vertex */
#define QRGPU_PP_NAN          0x20   /* a non-finite poseDest (or quaternion, base position, foot position, ground pitch); nothing is written */
#define QRGPU_PP_MAXITER      0x40   /* a QP was stopped after 200 active-set steps, a bound the reference does not have (set with INFEASIBLE) */
typedef struct {
    float rBH[12];                    /* the planner's own hip offsets (qr_pose_planner.cpp:48-50), not the robot's */
    float l_min, l_max, omega, eps;   /* leg-length window, weight of the support-polygon term, shrink of the polygon */
    float body_height;                /* bodyHight = A1_BODY_HIGHT */
    int   loops;                      /* SQP iterations */
} qrgpu_pose_plan_desc;
/* (+-0.18, +-0.047, 0), 0.22, 0.35, 0.5, 0.1, 0.27, 20 */
void qrgpu_pose_plan_desc_default(qrgpu_pose_plan_desc *d);
int qrgpu_pose_plan_batch(qrgpu_ctx *ctx, int n, const qrgpu_pose_plan_desc *desc, int event, const int *d_event, int reset,
                          const float *d_est_in, const float *d_est_out, const float *d_ground_out, const float *d_rpy,
                          const float *d_walk_out, float *d_pose_state, float *d_stance_cmd, float *d_pose_out, int *d_pose_flags);

/* The tick's state arrays from the estimator's inputs and outputs: what SolveDenseMPC (qr_mpc_stance_leg_controller.cpp:385-399:
 * pos, baseVInWorldFrame, quat, baseWInWorldFrame, foot2ComInWorldFrame = baseRMat (footPositionsInBaseFrame - comOffset), rpy) and
 * qrWbcLocomotionController::UpdateModel (qr_wbc_locomotion_controller.cpp:136-156) read.  d_rpy [3][n] = GetBaseRollPitchYaw.
 * Either output may be NULL. */
int qrgpu_pack_state_batch(qrgpu_ctx *ctx, int n, const float com_offset[3], const float *d_est_in, const float *d_est_out, const float *d_rpy,
                           float *d_mpc_state, float *d_fb_state);

/* ---- the plant: forward dynamics, ground contact, one control tick of the simulated robot -------------------------------------------------
 * What turns the torque of tick t into the state of tick t + 1, so that a batch runs in closed loop on the device.  The model is the one
 * qrgpu_wbc_setup uploads per type (base, 12 links, 12 rotors: BuildDynamicModel); both calls need a type set up there and follow the WBC's
 * rule for d_type_id (QRGPU_ERR_NOT_SETUP when no type was set up; a robot with a bad id is computed with the first valid type and flagged).
 *
 * qrgpu_forward_dynamics_batch: FloatingBaseModel::runABA with _externalForces (floating_base_model.cpp:876-947), rotor terms included.
 *   d_fb_state [37][n], d_tau [12][n], d_foot_force [12][n] (world-frame force on each foot point, 3*leg+axis; NULL = none)
 *   d_nu_dot [18][n]: the time derivative of the components of (omega_body, v_body, qd): dBodyVelocity and qdd.  It satisfies
 *   H nu_dot + C + G = [0; tau] + sum_leg Jc^T f.  The quaternion is normalised in fp64 on entry; arithmetic is fp64.
 *
 * qrgpu_plant_step_batch: d_fb_state advances in place by one control tick of params->substeps sub-steps of h = dt / substeps, each:
 *   motor law (the Gazebo joint controller's): tau = clip(Kp (p - q) + Kd (d - qd) + tua, +-tau_max) from d_motor_cmd [QRGPU_MOTOR_CMD_ROWS][n]
 *   contact law (OURS: the reference leaves the ground to its simulator): flat ground at ground_z; for a foot depth delta = ground_z - p_z > 0
 *     f_n = max(0, contact_k delta (1 - contact_a v_z)),  f_t = -mu f_n v_t / sqrt(|v_t|^2 + v_eps^2);  zero otherwise (continuous in the state)
 *   forward dynamics as above; semi-implicit Euler: nu += h nu_dot; q += h qd (new); pos += h R v_body (new v_body, R before the attitude
 *     update); quat <- normalise(quat (x) exp(h omega_body)) (new omega_body)
 *   The state is held in fp64 across the sub-steps: read once, written once as float32.
 * Outputs, each may be NULL:
 *   d_plant_out [QRGPU_PLANT_OUT_ROWS][n]: of the last sub-step foot force (world) [12], contact flag [4] (f_n > contact_threshold), applied
 *     torque [12] and nu_dot [18], at rows 0, 24, 28, 40; of the state written, foot position (world) [12] at row 12
 *   d_mpc_state [28][n]: the ground truth in qrgpu_pack_state_batch's conventions (foot vectors R (foot_b - com_offset); roll, pitch, yaw of
 *     the float32 quaternion written)
 *   d_est_in: rows 0-40 of est_in [54][n] without ReceiveObservation's filters: accelerometer (specific force at the base origin over the last
 *     sub-step, base frame), baseLinearAcceleration (the same), quaternion, gyro, foot contact, q, qd.  Rows 41-53 are left alone.
 *   d_status [n]: QRGPU_PL_* bits, 0 = fine.
 * QRGPU_ERR_BAD_ARG (nothing launched): n < 1 or n > max_batch, a NULL required array, substeps outside 1..64, dt <= 0.
 * Each call is one launch on the context's stream. */
#define QRGPU_PLANT_OUT_ROWS 58
#define QRGPU_PL_NONFINITE  0x1          /* a component of the result is not finite */
#define QRGPU_PL_QUAT_ZERO  0x2          /* the quaternion read was zero or not finite: the identity was used */
#define QRGPU_PL_BAD_TYPE   0x01000000   /* as QRGPU_ST_BAD_TYPE */
typedef struct {
    float dt;                   /* control tick, s */
    int substeps;               /* 1..64 */
    float contact_k;            /* N/m */
    float contact_a;            /* s/m */
    float mu;
    float v_eps;                /* m/s */
    float ground_z;
    float tau_max;              /* N m */
    float contact_threshold;    /* N */
    float com_offset[3];
} qrgpu_plant_params;
void qrgpu_plant_params_default(qrgpu_plant_params *p);     /* 0.002, 2, 2e4, 1.0, 0.6, 0.01, 0, 33.5, 5.0, A1's com offset */
int qrgpu_forward_dynamics_batch(qrgpu_ctx *ctx, int n, const int *d_type_id, const float *d_fb_state, const float *d_tau,
                                 const float *d_foot_force, float *d_nu_dot, int *d_status);
int qrgpu_plant_step_batch(qrgpu_ctx *ctx, int n, const qrgpu_plant_params *params, const int *d_type_id, float *d_fb_state,
                           const float *d_motor_cmd, float *d_plant_out, float *d_mpc_state, float *d_est_in, int *d_status);

/* qrgpu_plant_step_terrain_batch: qrgpu_plant_step_batch on a ground that is a height field chosen per robot, with a push on the base held
 * for the tick.  qrgpu_plant_step_batch itself is untouched: the flat call computes what it computed.
 *   Field: d_height holds terrain->n_fields grids of ny x nx float32 heights, x fastest (d_height[f][j][i]); node (i, j) lies at
 *     (x0 + i cell, y0 + j cell).  Robot r stands on field d_field_id[r] (NULL: every robot on field 0).
 *   Sampler: bicubic Catmull-Rom (cubic convolution, a = -1/2), separable, on the heights widened to fp64.  u = (x - x0) / cell clipped to
 *     [0, nx - 1]; i = min(floor(u), nx - 2), t = u - i; weights w(t) = 1/2 (-t^3 + 2 t^2 - t, 3 t^3 - 5 t^2 + 2, -3 t^3 + 4 t^2 + t, t^3 - t^2)
 *     on the nodes i - 1 .. i + 2, each index clamped to [0, nx - 1]; the same in y.  The slopes dz/dx, dz/dy come from the derivative weights
 *     w'(t) / cell at the same clipped (u, v).  The surface is C1 (the cell on either side of a grid line gives the same height and normal);
 *     outside the grid it has the height and the normal of the nearest border point.
 *   Contact law, for a foot at world p with velocity v:  z_g = sampled height + params->ground_z;  n = (-z_x, -z_y, 1) / |.|;
 *     delta = (z_g - p_z) n_z;  v_n = v . n,  v_t = v - v_n n;  f_n = max(0, contact_k delta (1 - contact_a v_n)) for delta > 0, else 0;
 *     f = f_n n - mu f_n v_t / sqrt(|v_t|^2 + v_eps^2).  On a constant field this is qrgpu_plant_step_batch's law.
 *   Push: d_base_push [6][n] = a world-frame force acting at the base origin (rows 0-2) and a world-frame moment (rows 3-5), held over the
 *     tick; every sub-step rotates them into the base frame and adds [R^T moment; R^T force] to the right-hand side of the base's rows:
 *     H nu_dot + C + G = [0; tau] + sum_leg Jc^T f + [R^T moment; R^T force; 0].  NULL = none.
 *   d_terrain_out [QRGPU_TERRAIN_OUT_ROWS][n] (may be NULL): of the state written, per foot, the ground height z_g under the foot [4] at row 0
 *     and the unit normal there [12] (3 * leg + axis) at row 4.
 *   d_status: the QRGPU_PL_* bits of qrgpu_plant_step_batch and the two below.
 * The other arguments, outputs and rules are qrgpu_plant_step_batch's.  QRGPU_ERR_BAD_ARG (nothing launched) also for a NULL terrain or
 * d_height, nx or ny < 2, n_fields < 1, cell <= 0 or not finite, x0 or y0 not finite.  One launch on the context's stream. */
struct qrgpu_terrain_desc { int nx, ny, n_fields; float x0, y0, cell; };
typedef struct qrgpu_terrain_desc qrgpu_terrain_desc;
#define QRGPU_TERRAIN_OUT_ROWS 16       /* per foot: ground height under the foot [4] at row 0, unit normal [12] at row 4, of the state written */
#define QRGPU_PL_BAD_FIELD 0x4          /* d_field_id outside 0..n_fields-1: field 0 was used */
#define QRGPU_PL_OFF_FIELD 0x8          /* a foot (the body call: any point) with f_n > 0 outside the grid in the last sub-step: the border was extended */
int qrgpu_plant_step_terrain_batch(qrgpu_ctx *ctx, int n, const qrgpu_plant_params *params, const qrgpu_terrain_desc *terrain,
                                   const float *d_height, const int *d_field_id /* [n], NULL = field 0 */,
                                   const float *d_base_push /* [6][n] force, moment; NULL = none */, const int *d_type_id, float *d_fb_state,
                                   const float *d_motor_cmd, float *d_plant_out, float *d_terrain_out, float *d_mpc_state, float *d_est_in,
                                   int *d_status);

/* qrgpu_plant_step_body_batch: qrgpu_plant_step_terrain_batch for a robot that has a body -- it touches the ground with its knees and its trunk
 * as well as its feet, and its joints have stops.  A robot that loses its footing comes to rest on the ground, finite, and says so in d_status.
 * The flat and the terrain call are untouched: they compute what they computed.
 *   Points: a robot has 16 contact points.  Per leg l (FR FL RR RL, signs sx, sy as for the abad location): the foot, as in the other calls; the
 *     knee, the origin of the knee link's frame, with that origin's velocity; and the two trunk corners on the leg's side,
 *     trunk_center + (sx hx, sy hy, -+hz) in the base frame, moving with the base (the four top corners carry a robot on its back).
 *   Every point takes the terrain call's law unchanged: the surface sampled at the point's world x, y, z_g = sampled height + ground_z, and
 *     f = f_n n - mu f_n v_t / sqrt(|v_t|^2 + v_eps^2) with the call's contact_k, contact_a, mu, v_eps.  Points, no radii; no new contact parameter.
 *   Joint limits, per joint with lo = q_lo, hi = q_hi of its kind (abad, hip, knee), k_l = limit_k, a_l = limit_a:
 *     tau_lim = -max(0, k_l (q - hi) (1 + a_l qd)) for q > hi,  +max(0, k_l (lo - q) (1 - a_l qd)) for q < lo,  0 otherwise:
 *     one-sided and continuous in the state, like the contact law.  It is added to the joint torque AFTER the motor law's clip: a stop is not
 *     the motor.
 *   Each sub-step:  H nu_dot + C + G = [0; tau_motor + tau_lim] + sum_feet Jc^T f + sum_knees Jk^T f_k + sum_corners Jc^T f_c
 *     + [R^T moment; R^T force; 0], with the field, the per-robot field id, the push, the integrator and the fp64 state of the terrain call.
 *   Per type: qrgpu_plant_body_setup keeps one qrgpu_plant_body_desc per type_id beside the model constants of qrgpu_wbc_setup.
 *     QRGPU_ERR_BAD_ARG for a non-finite or non-positive trunk_half, a non-finite trunk_center or limit, q_lo >= q_hi, a negative or non-finite
 *     limit_k or limit_a.
 *   d_plant_out, d_terrain_out, d_mpc_state, d_est_in: the terrain call's (the torque rows of d_plant_out hold the motor's torque).
 *   d_body_out [QRGPU_BODY_OUT_ROWS][n] (may be NULL), of the last sub-step: knee force, world frame [12] (3 * leg + axis) at row 0; knee
 *     contact flag [4] (f_n > contact_threshold) at row 12; the corners' f_n [8] (2 * leg + top) at row 16; tau_lim [12] at row 24.
 *   d_status: the terrain call's bits and the three below; QRGPU_PL_OFF_FIELD here means ANY point with f_n > 0 outside the grid.
 * QRGPU_ERR_BAD_ARG as the terrain call; QRGPU_ERR_NOT_SETUP also unless every type set up with qrgpu_wbc_setup has a body desc.  One launch on
 * the context's stream.
 *
 * Defaults of the stops.  The integrator is semi-implicit Euler, stable on an oscillator for omega h < 2; omega h <= 0.2 keeps a stop's
 * frequency error under one percent.  The stiffest oscillator a stop can meet is the joint with the smallest reflected inertia, the knee: the knee
 * link about its axis, I_yy + m (c_x^2 + c_z^2) = 3014e-6 + 0.166 (0.006435^2 + 0.107^2) = 4.92e-3 kg m^2, plus k_rot^2 times the rotor's 1e-8
 * (gear ratio 1: nothing).  At the default sub-step h = 1 ms, omega <= 200 rad/s gives k_l <= 4.92e-3 * 200^2 = 197 N m/rad; the default is
 * limit_k = 150 (omega h = 0.175; the motor's 33.5 N m hold a joint 0.22 rad beyond its stop).  The damping rate a stop adds is
 * k_l a_l x / I at excursion x; with limit_a = 0.02 s/rad it is 0.3 / h at x = 0.5 rad, well inside the integrator's bound of 2 / h. */
struct qrgpu_plant_body_desc {
    float trunk_half[3];        /* hx, hy, hz of the trunk box, m */
    float trunk_center[3];      /* its centre in the base frame */
    float q_lo[3], q_hi[3];     /* joint limits of abad, hip, knee, rad, in this library's sign convention (stand pose 0, 0.8, -1.6) */
    float limit_k;              /* N m / rad */
    float limit_a;              /* s / rad */
};
typedef struct qrgpu_plant_body_desc qrgpu_plant_body_desc;
#define QRGPU_BODY_OUT_ROWS 36
#define QRGPU_PL_TRUNK_CONTACT 0x10     /* a trunk corner with f_n > contact_threshold in the last sub-step */
#define QRGPU_PL_KNEE_CONTACT  0x20     /* a knee with f_n > contact_threshold in the last sub-step */
#define QRGPU_PL_JOINT_LIMIT   0x40     /* a joint beyond a stop (tau_lim != 0) in the last sub-step */
/* A1: a1_description's trunk box 0.267 x 0.194 x 0.114 at the base origin; limits +-46 deg, -60..240 deg, -154.5..-52.5 deg; 150, 0.02 */
void qrgpu_plant_body_desc_default(qrgpu_plant_body_desc *desc);
int qrgpu_plant_body_setup(qrgpu_ctx *ctx, int type_id, const qrgpu_plant_body_desc *desc);
int qrgpu_plant_step_body_batch(qrgpu_ctx *ctx, int n, const qrgpu_plant_params *params, const qrgpu_terrain_desc *terrain,
                                const float *d_height, const int *d_field_id /* [n], NULL = field 0 */,
                                const float *d_base_push /* [6][n] force, moment; NULL = none */, const int *d_type_id, float *d_fb_state,
                                const float *d_motor_cmd, float *d_plant_out, float *d_terrain_out, float *d_body_out, float *d_mpc_state,
                                float *d_est_in, int *d_status);

/* ---- episodes: per-robot termination, reset and spawn on the device ---------------------------------------------------------------------------
 * qrgpu_episode_step_batch decides for every robot whether its episode ends at this call and, where it does, closes the episode's statistics and
 * writes the robot's next spawn into d_fb_state -- no host copy, no host decision.  One memset (of d_done_count) and one launch on the context's
 * stream.  It changes no other call.
 *
 * Termination: d_done [n] gets the robot's QRGPU_EP_* reason bits, every call; (d_done & QRGPU_EP_REASONS) == 0: the episode goes on.  All bits
 * that apply are set.
 *   EP_STATUS       d_plant_status[r] & status_mask was non-zero at this and the previous status_ticks - 1 calls (a per-robot counter in
 *                   d_ep_state debounces it; the counter is cleared by a call that finds the masked status 0).  NULL array: never.
 *   EP_TICK_STATUS  d_tick_status[r] & tick_mask is non-zero.  NULL array: never.
 *   EP_NONFINITE    one of the robot's 37 d_fb_state rows is not finite.  Judged here, on the rows themselves.  The four geometric tests below are
 *                   then not made (their bits stay 0): no comparison with a NaN decides a bit.
 *   EP_TILT         R_zz = 1 - 2 (q_x^2 + q_y^2) / |q|^2 (fp64) < cos(tilt_max); tilt_max >= pi (as a float): never.  A zero quaternion is read as the identity, as
 *                   the plant reads it.
 *   EP_HEIGHT       base z - ground height under the base origin < min_clearance; ground height = the robot's field sampled at the base x, y
 *                   (the sampler of qrgpu_plant_step_terrain_batch) + params->ground_z; without a terrain, params->ground_z (params NULL: 0).
 *   EP_OFF_FIELD    with a terrain only: the base x, y lies outside [x0 + field_margin, x0 + (nx - 1) cell - field_margin] x (the same in y).
 *   EP_TIMEOUT      the episode's tick count has reached max_ticks (0: never).  A truncation, not a failure.  The count is the number of calls
 *                   since the one that spawned the episode, this one included: with one plant step between calls, the plant steps it ran.
 *   EP_FORCED       d_force_reset[r] != 0 (NULL array: never), and every robot of a call with reset_all != 0.
 *   QRGPU_EP_BAD_FIELD is no reason: with a terrain, d_field_id[r] outside 0..n_fields-1 -- field 0 was used (the rule of QRGPU_PL_BAD_FIELD).
 *
 * Random numbers: Philox-4x32-10, key (seed, robot index), counter (episode index, block k, 0, 0); uniform u = (word >> 8) 2^-24 in [0, 1), exact
 * in float, widened to fp64; s = 2 u - 1.  A spawn depends on (seed, robot, episode index) alone -- not on n, the launch or the history.
 * Draw order:  block 0: words 0..3 = spawn-table row, dx, dy, dyaw;  block 1: words 0, 1 = v_x, v_y (2, 3 unused);  block 2 + b, word j = joint
 * 4 b + j (b = 0..2).
 *
 * Spawn, from d_spawn [4][n_spawn] (rows x, y, yaw, reserved):  row = min(floor(u n_spawn), n_spawn - 1);  x = x_row + xy_jitter s, y likewise,
 * yaw = yaw_row + yaw_jitter s.  Ground height z_g and unit normal nrm of the robot's field at (x, y) as above (no terrain: ground_z, (0, 0, 1)).
 * Base position (x, y, z_g) + spawn_height nrm.  Attitude: align_to_slope != 0: q_tilt (x) q_yaw with q_tilt = (1 + nrm_z, -nrm_y, nrm_x, 0) /
 * |.| (the shortest rotation of e_z onto nrm: the base z axis is nrm) and q_yaw = (cos yaw/2, 0, 0, sin yaw/2); otherwise q_yaw.  Written
 * normalised with w >= 0.  Joints q_spawn[j] + q_jitter s; v_body x, y = v_jitter s; every other velocity 0.
 *
 * Bookkeeping.  d_ep_state [QRGPU_EPISODE_STATE_ROWS][n] int32: 0 ticks in this episode, 1 episode index, 2 status debounce counter, 3 reason of
 * the last episode ended, 4 episodes ended with any bit other than EP_TIMEOUT, 5 episodes ended by EP_TIMEOUT alone.
 * d_ep_stats [QRGPU_EPISODE_STATS_ROWS][n] float: 0-3 spawn x, y, z, yaw of the running episode (the base position written); of the last
 * episode ended: 4 its length in ticks, 5, 6 its world displacement x - spawn x, y - spawn y (0 for a robot with EP_NONFINITE), 7 its minimum
 * clearance; 8 the running minimum of the clearance judged at each call (started at spawn_height; a call with EP_NONFINITE leaves it).
 * reset_all != 0: every robot starts episode 0 as on fresh arrays -- rows zeroed, spawned, d_done = EP_FORCED, nothing closed or counted; what
 * d_ep_state, d_ep_stats and d_fb_state held is not read.  The first call on new arrays is such a call -- or the caller, who wants the
 * robots to start where they stand, zeroes d_ep_state and writes rows 0-3 and 8 of d_ep_stats itself.
 *
 * A robot that is reset gets: its 37 d_fb_state rows; d_prev_ori rows 0 (if given); its d_motor_cmd column (if given) as a joint PD hold at the
 * joints drawn: p = q, Kp = kp, d = 0, Kd = kd, tua = 0 -- the next plant step does not apply a torque computed for the fallen pose.  Of a robot
 * that is not reset only rows 0 and 2 of d_ep_state and row 8 of d_ep_stats are written.
 * d_done_list [n] (may be NULL): the indices of the robots reset in this call; d_done_count [1]: how many (required with d_done_list, may be given
 * alone).  THE ORDER OF THE LIST IS UNSPECIFIED across wavefronts (ascending inside one): each wavefront with a reset claims its span with one
 * atomic add.
 *
 * Contracts.
 *   Order: the intended loop is episode step, plant step, tick.  The plant step that follows a reset writes mpc_state, est_in and plant_out of
 *     the new state, so this call writes none of them; a robot's first tick after a reset is computed from its post-reset state.
 *   Warm start: a robot's stored MPC working set is not cleared: it is speed only (qrgpu_set_warm_start), a stale set leaves row by row.
 *   Overlapped ticks: this call is "another launch of the context" -- the next tick is not chained (qrgpu_set_tick_overlap, rule 2).  It does not
 *     touch the hand-over words of prev_ori.
 *   Stage memory: the controller stages in front of the tick reset a robot of their own accord when bound to d_done and d_ep_state with
 *     qrgpu_set_stage_reset (below).  The loop is then: episode step, plant step, ground, estimator, gait, swing, front-end or stance, tick.
 * QRGPU_ERR_BAD_ARG (nothing launched; qrgpu_last_error names the argument): n < 1 or n > max_batch; NULL desc, d_fb_state, d_ep_state,
 * d_ep_stats, d_done or d_spawn; n_spawn < 1; a terrain the terrain call would refuse (nx or ny < 2, n_fields < 1, cell <= 0 or not finite, x0 or y0 not finite), or a terrain without
 * d_height; d_done_list without
 * d_done_count; status_ticks < 1, max_ticks < 0; a negative or non-finite tilt_max, min_clearance, field_margin, spawn_height, jitter, kp or kd;
 * a non-finite q_spawn. */
#define QRGPU_EP_STATUS       0x1
#define QRGPU_EP_TICK_STATUS  0x2
#define QRGPU_EP_NONFINITE    0x4
#define QRGPU_EP_TILT         0x8
#define QRGPU_EP_HEIGHT       0x10
#define QRGPU_EP_OFF_FIELD    0x20
#define QRGPU_EP_TIMEOUT      0x40
#define QRGPU_EP_FORCED       0x80
#define QRGPU_EP_REASONS      0xff          /* a robot is reset when (d_done & QRGPU_EP_REASONS) != 0 */
#define QRGPU_EP_BAD_FIELD    0x01000000    /* not a reason: d_field_id outside the stack, field 0 was used */
#define QRGPU_EPISODE_STATE_ROWS 6
#define QRGPU_EPISODE_STATS_ROWS 9
struct qrgpu_episode_desc {
    int   status_mask;          /* QRGPU_PL_* bits of d_plant_status that end an episode */
    int   status_ticks;         /* ... after this many consecutive calls, >= 1 */
    int   tick_mask;            /* bits of d_tick_status that end an episode */
    int   max_ticks;            /* 0 = no timeout */
    unsigned seed;
    int   align_to_slope;
    float tilt_max;             /* rad */
    float min_clearance;        /* m */
    float field_margin;         /* m */
    float spawn_height;         /* m, along the ground's normal */
    float xy_jitter, yaw_jitter, q_jitter, v_jitter;     /* +- m, rad, rad, m/s */
    float q_spawn[12];
    float kp, kd;               /* the PD hold written into d_motor_cmd */
};
typedef struct qrgpu_episode_desc qrgpu_episode_desc;
/* PL_NONFINITE | PL_QUAT_ZERO | PL_TRUNK_CONTACT, 1, 0, 0, seed 1, level, 1.0, 0.10, 0, 0.30, jitters 0, (0, 0.8, -1.6) per leg, 100, 2 */
void qrgpu_episode_desc_default(qrgpu_episode_desc *d);
int  qrgpu_episode_step_batch(qrgpu_ctx *ctx, int n, const qrgpu_episode_desc *desc, int reset_all, const qrgpu_plant_params *params,
                              const qrgpu_terrain_desc *terrain /* NULL = flat at ground_z */, const float *d_height,
                              const int *d_field_id /* [n], NULL = field 0 */, const float *d_spawn /* [4][n_spawn] */, int n_spawn,
                              const int *d_plant_status, const int *d_tick_status, const int *d_force_reset, float *d_fb_state,
                              float *d_prev_ori, float *d_motor_cmd, int *d_ep_state, float *d_ep_stats, int *d_done, int *d_done_list,
                              int *d_done_count);

/* ---- per-robot reset and clock of the stage kernels -------------------------------------------------------------------------------------------
 * qrgpu_set_stage_reset binds the stages with memory to a device mask and a device tick count, so that a robot that qrgpu_episode_step_batch has
 * respawned starts its gait, swing, estimator, ground, stance, pose-planner and front-end memory afresh at its next stage calls, with a clock of
 * its own -- in the reference qrLocomotionController::Reset restarts timeSinceReset (qr_locomotion_controller.cpp:56-66), which Update feeds to the
 * gait generator (:69-76): time is per robot.  Off by default; r == NULL switches it off.  The struct is copied; the arrays are read when the
 * kernels run on the context's stream, not at this call: an episode step queued before the stage calls is ordered before them.  With
 * d_mask = d_done, bits = QRGPU_EP_REASONS, d_ticks = d_ep_state (row 0: ticks in this episode) and tick_dt the control period, the loop is
 *     episode step, plant step, ground, estimator, gait, swing, front-end or stance, tick.
 * While a binding is set, robot r's reset level at a stage call is the call's scalar `reset` if that is non-zero (exactly as without a binding);
 * otherwise the bound level if (d_mask[r] & bits) != 0; otherwise 0.  The bound level in each stage's own numbers:
 *     stage                                              CONSTRUCT   LIVE
 *     qrgpu_gait_update_batch                            1           2
 *     qrgpu_walk_gait_update_batch                       2           1
 *     qrgpu_swing_update_batch                           2           1
 *     ground, stance update / tick, pose plan            their one level
 * What a scalar reset writes beside the state (d_swing_flags cleared, the lift-off rows of d_swing_in, d_swing_vel_in and d_fe_in, d_stance_state
 * at body_height) a masked robot gets in the same way.  qrgpu_pose_plan_batch launches for a masked robot also where event is 0.
 * The two stages without a scalar reset:
 *     qrgpu_estimator_update_batch   a masked robot's d_est_state column is taken as zeros (its content is not read); the update goes on from there.
 *     qrgpu_mpc_frontend_batch       a masked robot's d_fe_state column gets MPCStanceLegController::Reset (qr_mpc_stance_leg_controller.cpp:78-81,
 *                                    :92) before the update: row 2 = 0, row 3 = fe_in row 9, rows 4-6 = fe_in rows 6-8, row 7 = 0; rows 0, 1 are
 *                                    kept at LIVE and 0 at CONSTRUCT (the members' initialisers, qr_mpc_stance_leg_controller.h:126,131).
 * With d_ticks, qrgpu_gait_update_batch, qrgpu_walk_gait_update_batch, qrgpu_stance_update_batch and qrgpu_stance_tick_batch use
 * current_time_r = (float)d_ticks[r] * tick_dt (one float product) where they use the scalar current_time, which is then ignored;
 * desc->pose_reset_time of the stance stage stays scalar.  qrgpu_observe_batch (below) reads the mask, not d_ticks: a masked robot starts from a zero
 * d_obs_state column, as under its scalar reset; so do qrgpu_command_update_batch (d_cmd_state) and qrgpu_mpc_command_batch (d_cmd_mem), further below.
 * No other entry point reads the binding: not the pack, footholds, swing targets, swing
 * velocity, swing action and stance command calls, the tick, the plant or the episode step.
 * QRGPU_ERR_BAD_ARG (nothing changed: an earlier binding stays in force; qrgpu_last_error names the field): d_mask and d_ticks both NULL; d_mask
 * with bits == 0; d_mask with a level that is neither of the two; d_ticks with a tick_dt that is not finite or not greater than 0. */
#define QRGPU_STAGE_RESET_CONSTRUCT 1   /* the stage as constructed, then its Reset() */
#define QRGPU_STAGE_RESET_LIVE      2   /* Reset() on the running stage */
typedef struct {
    const int *d_mask;    /* [n] or NULL; robot r is reset at a stage call when (d_mask[r] & bits) != 0 */
    unsigned   bits;      /* e.g. QRGPU_EP_REASONS with d_mask = d_done */
    int        level;     /* one of the two above */
    const int *d_ticks;   /* [n] or NULL; per-robot clock: current_time_r = (float)d_ticks[r] * tick_dt, one float32 product */
    float      tick_dt;   /* e.g. 0.002f with d_ticks = d_ep_state (row 0: ticks in this episode) */
} qrgpu_stage_reset;
int qrgpu_set_stage_reset(qrgpu_ctx *ctx, const qrgpu_stage_reset *r /* NULL: off */);

/* ---- the sensor stage: qrRobot*::ReceiveObservation on the device ------------------------------------------------------------------------------
 * qrgpu_observe_batch turns the raw sensor rows a plant call writes (rows 0-40 of est_in "without ReceiveObservation's filters") into what the
 * estimator chain reads per tick -- the filtered rows of est_in, d_rpy for qrgpu_pack_state_batch, d_ground_in for qrgpu_ground_update_batch, d_tick
 * for qrgpu_estimator_update_batch -- so that plant, observe, ground, estimator, pack, tick run without the host touching a robot.  One launch on
 * the context's stream, one lane per robot.  It changes no other call.  The reference: qr_robot_a1_sim.cpp:606-670 (qrRobotSim: qr_robot_sim.cpp:547-),
 * qr_robot_a1.cpp:140-193; the filters qr_robot.cpp:30-37, their Reset :55-58; qrMovingWindowFilter<float, N> qr_moving_window_filter.hpp:139-189.
 * Arithmetic is float32 where the reference's is, its double literals promoting where they do there, contraction off.
 *
 * Per robot, in this order (d_raw rows as qrgpu_plant_step_batch's d_est_in; rows 3-5 of d_raw are not read):
 *   noise (OURS; the reference has none): row += amplitude * s, one float product and one float sum, s = 2 u - 1, u = (word >> 8) 2^-24 from
 *     Philox-4x32-10 with key (seed, robot index) and counter (step, block, 0x0b5e7, 0).  Block 0, words 0-2: accelerometer x, y, z; block 1, words
 *     0-2: gyro; blocks 2-4, word j of block 2 + b: q of joint 4 b + j; blocks 5-7: qd likewise.  An amplitude of 0 skips the add: the row's bits are
 *     those read.  The noise depends on (seed, robot, step) alone -- not on the history, n or the launch; step is the caller's loop count.  The
 *     attitude carries no noise.
 *   est_in rows 0-2    the (noised) accelerometer, baseAccInBaseFrame
 *   est_in rows 3-5    accFilter.CalculateAverage of it: window 5, Neumaier sum with its correction, divided by the length after the push
 *   roll, pitch, yaw   raw = quatToRPY(d_raw rows 6-9) (state.imu.rpy); calibratedYaw = yaw - yaw_offset, -= M_2PI where >= M_PI, += M_2PI where
 *                      <= -M_PI (M_2PI is the reference's 6.28318530718, qr_ctypes.h:51).  filter_rpy != 0 (the sim classes): if
 *                      |baseRollPitchYaw[2] of the previous call - calibratedYaw| >= M_PI the rpy filter is cleared (rpyFilter.Reset()); then
 *                      rpyFilter.CalculateAverage (window 5) of (roll, pitch, calibratedYaw); then the averaged yaw is folded in the same way.
 *                      filter_rpy == 0 (the hardware classes): (roll, pitch, calibratedYaw) as it is.
 *   d_rpy [3][n]       that baseRollPitchYaw
 *   est_in rows 6-9    baseOrientation = rpyToQuat(baseRollPitchYaw) = rotationMatrixToQuaternion(rpyToRotMat(.)) in float (qr_se3.h:145-178, 228-235)
 *   est_in rows 10-12  gyroFilter.CalculateAverage (window 5) of the (noised) gyro
 *   est_in rows 13-16  foot contacts, copied: the plant's contact_threshold default of 5 N is the sim classes' footForce >= 5
 *                      (qr_robot_a1_sim.cpp:662; the hardware class compares with 15, qr_robot_a1.cpp:183: set contact_threshold)
 *   est_in rows 17-28  the (noised) q, copied
 *   est_in rows 29-40  the (noised) qd: filter_motor_velocity != 0 (the hardware classes) through motorVFilter, a 12-vector window of 20
 *                      (qr_robot_a1.cpp:176); otherwise copied
 *   est_in rows 41-53  never written: they belong to the gait (41-44) and to qrgpu_ground_update_batch (45-53)
 *   d_ground_in [23][n] (may be NULL)  rows 0-3 the contacts of this tick; 4-15 FootPositionsInBaseFrame(q) of this tick's angles (UpdateDataFlow,
 *                      qr_robot.cpp:68; hip_l, upper_l, lower_l, hip_offset as in qrgpu_estimator_desc); 16-18 basePosition = rows 36-38 of
 *                      d_est_out_prev, the estimator's output of the previous tick -- (0, 0, base_height) when that array is NULL or the robot is
 *                      reset at this call (qrRobot::Reset, qr_robot.cpp:53); 19-22 the quaternion of rows 6-9
 *   d_tick [n] (may be NULL)  count * tick_ms, count = the robot's calls since its reset, this one included: the first call gives tick_ms, never 0
 *                      (the estimators take a last timestamp of 0 for "first sample")
 * Deliberate readings: abs(baseRollPitchYaw[2] - calibratedYaw) (qr_robot_a1_sim.cpp:630) is read as std::abs(float), the project's standing
 * reading of the reference's unqualified abs; the hardware class's groundPitch (qr_robot_a1.cpp:160) is computed there and never used; the
 * motor torques, accelerations and ComputeMoment of UpdateDataFlow feed nothing the library runs and are not produced.
 *
 * d_obs_state [qrgpu_observe_state_rows(desc)][n] float32, the stage's memory (the filters are float in the reference: a float row holds them
 * exactly).  Zero = as constructed / after Reset().  Row 0: the call counter, an unsigned 32-bit integer in the row's bits.  Row 1: baseRollPitchYaw[2]
 * of the previous call.  Rows 2-24 accFilter, 25-47 gyroFilter, 48-70 rpyFilter, each: sum[3], correction[3], the deque's length, head (the ring slot
 * the next push writes), ring[5 slots][3 axes].  Rows 71-336, read, written and needed only with filter_motor_velocity: sum[12], correction[12],
 * length, head, ring[20 slots][12].  A length or head row that does not hold an integer of its range is read as 0.
 * reset != 0: every robot starts from a zero column; what the column held is not read, and it is zero before the call writes to it.  Under
 * qrgpu_set_stage_reset a robot with (d_mask[r] & bits) != 0 is reset in the same way when the scalar is 0; d_ticks is not read.
 * d_est_in may be d_raw itself (the plant's rows filtered in place): a lane loads all its raw rows before its first store.  No other two arrays
 * may overlap.
 * QRGPU_ERR_BAD_ARG (nothing launched; qrgpu_last_error names the argument): n < 1 or n > max_batch; a NULL desc, d_raw, d_obs_state, d_est_in or
 * d_rpy; tick_ms == 0; a negative or non-finite noise amplitude; a non-finite yaw_offset, base_height, hip_l, upper_l, lower_l or hip_offset. */
#define QRGPU_OBS_SIM      0            /* qrRobotA1Sim, qrRobotSim */
#define QRGPU_OBS_HARDWARE 1            /* qrRobotA1 */
#define QRGPU_OBSERVE_STATE_ROWS    71  /* without the motor-velocity window */
#define QRGPU_OBSERVE_STATE_ROWS_MV 337 /* with it */
struct qrgpu_observe_desc {
    int   filter_rpy;               /* sim classes: 1 (rpyFilter, with its Reset at a yaw jump >= pi); hardware classes: 0 */
    int   filter_motor_velocity;    /* hardware classes: 1 (window 20); sim classes: 0 */
    float yaw_offset;               /* yawOffset: 0 in the sim classes; the hardware class reads it at start-up (qr_robot_a1.cpp:133) */
    float hip_l, upper_l, lower_l;  /* FootPositionsInBaseFrame, as qrgpu_estimator_desc */
    float hip_offset[12];
    float base_height;              /* qrRobot::Reset basePosition z: A1_BODY_HIGHT 0.27 */
    unsigned tick_ms;               /* milliseconds per call: 2 */
    unsigned seed;                  /* sensor noise, OURS */
    float acc_noise, gyro_noise, q_noise, qd_noise;     /* amplitudes, m/s^2, rad/s, rad, rad/s; 0 = none */
};
typedef struct qrgpu_observe_desc qrgpu_observe_desc;
/* variant QRGPU_OBS_SIM: 1, 0; QRGPU_OBS_HARDWARE: 0, 1; both: 0, A1's geometry (0.08505, 0.2, 0.2, (+-0.1805, +-0.047, 0)), 0.27, 2, seed 1, no noise */
void qrgpu_observe_desc_default(qrgpu_observe_desc *d, int variant);
int  qrgpu_observe_state_rows(const qrgpu_observe_desc *d);      /* rows of d_obs_state; 0 for NULL */
int  qrgpu_observe_batch(qrgpu_ctx *ctx, int n, const qrgpu_observe_desc *desc, int reset, unsigned step,
                         const float *d_raw /* [41][n]: rows 0-40 as the plant writes them */,
                         const float *d_est_out_prev /* [42][n] of the previous tick, or NULL */, float *d_obs_state,
                         float *d_est_in /* [54][n]; may be d_raw itself */, float *d_rpy /* [3][n] */,
                         float *d_ground_in /* [23][n], may be NULL */, unsigned *d_tick /* [n], may be NULL */);

/* ---- the trot's command, data-flow and motor-command stages --------------------------------------------------------------------------------------
 * The three pieces of the reference that lie between the stage kernels of the MPC trot (LocomotionMode::ADVANCED_TROT with MPC + WBC).  With them a
 * trot tick is queued on the context's stream with no host copy: [episode step,] plant, observe, ground, estimator, pack, command, gait (d_contact =
 * rows 13-16 of est_in), trot inputs, swing update, footholds, swing targets, MPC front-end, tick, MPC command (tools/closed_loop.py --trot).
 * One launch each, one lane per robot, float32 where the reference is float32, its double literals promoting where they do there, contraction off.
 * QRGPU_ERR_BAD_ARG (nothing launched, outputs untouched; qrgpu_last_error names the argument): a NULL required array or desc, n < 1, n > max_batch,
 * a reset other than 0 or 1.
 *
 * qrgpu_command_update_batch: qrDesiredStateCommand::Update (QS/controllers/qr_desired_state_command.cpp:164-265).
 *   d_joy [QRGPU_JOY_ROWS][n]  0-2 joyCmdVx, Vy, Vz; 3-5 joyCmdRollRate, PitchRate, YawRate (already scaled, as the members are); 6 joycmdBodyHeight;
 *                      7 joyCtrlState, an RC_MODE value as a float (HARD_CODE 0, JOY_TROT 1, JOY_ADVANCED_TROT 2, JOY_WALK 3, JOY_STAND 4, BODY_UP 5,
 *                      BODY_DOWN 6, EXIT 7; anything else is read as EXIT).  The button state machine (JoyCallback, and the joyCtrlStateChangeRequest
 *                      block of Update, :173-211) is per event and stays with the caller, who supplies the resulting mode.  In HARD_CODE rows 0-2 and
 *                      3-5 are vDesInBodyFrame / wDesInBodyFrame, taken unfiltered.  The rows are not written: the zeros JOY_STAND assigns to the
 *                      joyCmd members are the next JoyCallback's to overwrite.
 *   d_cmd_state [QRGPU_CMD_STATE_ROWS][n]  the stage's memory: filteredVel[3], filteredOmega[3].  reset 1: every robot starts from zeros (as
 *                      constructed, :36-37); under qrgpu_set_stage_reset a robot with (d_mask[r] & bits) != 0 does so when the scalar is 0.
 *   d_state_des [12][n] stateDes.  As written in the reference: (0), (1) and (5) are dt times entries of the vector just zeroed; (4) is
 *                      clip(filteredOmega[1] * dt, pitch); (2) is joycmdBodyHeight, times the double 0.85 where stateDes(6) < -0.01; the JOY_STAND and
 *                      else branches zero the filter state as well as the output; the filter is state * float(1.0 - filterFactor) + cmd * filterFactor.
 *   the rows the existing kernels read, no other row of those arrays touched: d_fe_in 0-5 (stateDes 2, 3, 4, 6, 7, 11), d_fh_in 16-20 (6, 7, 8, 11, 2),
 *                      d_swing_vel_in 23-26 (6, 7, 8, 11), d_stance_cmd 0-6 (2, 6, 7, 8, 9, 10, 11).  Each of the five outputs may be NULL.
 *   Rows 23-26 of d_swing_vel_in are not where qrgpu_swing_velocity_batch reads these values (yaw rate 23, desiredSpeed 24-26, desiredTwistingSpeed 27):
 *   the chain of the velocity mode passes d_swing_vel_in = NULL here and lets qrgpu_velocity_inputs_batch, which runs later, write rows 23-27. */
#define QRGPU_JOY_ROWS 8
#define QRGPU_CMD_STATE_ROWS 6
struct qrgpu_command_desc {
    float dt;                         /* qr_desired_state_command.hpp:155: 0.002 */
    float filter_factor;              /* :266: 0.02 */
    float body_height;                /* robot->bodyHeight, what joycmdBodyHeight is constructed with (qr_desired_state_command.cpp:49; a1_sim: 0.28):
                                         the value for row 6 of d_joy; the kernel reads the row */
    float min_velx, max_velx;         /* :317, :312: -0.15, 0.2 */
    float min_vely, max_vely;         /* :327, :322: -0.1, 0.1 */
    float min_yawrate, max_yawrate;   /* :337, :332: -0.2, 0.2 */
    float min_pitch, max_pitch;       /* :307, :302: -0.5, 0.5 */
};
typedef struct qrgpu_command_desc qrgpu_command_desc;
void qrgpu_command_desc_default(qrgpu_command_desc *d);
int  qrgpu_command_update_batch(qrgpu_ctx *ctx, int n, const qrgpu_command_desc *desc, int reset, const float *d_joy, float *d_cmd_state,
                                float *d_state_des, float *d_fe_in, float *d_fh_in, float *d_swing_vel_in, float *d_stance_cmd);

/* qrgpu_trot_inputs_batch: the getters of qrRobot / qrStateDataFlow / the gait generator that the trot's controllers call, from arrays the device holds.
 * Reads d_est_in (quat_wxyz 6-9, rpyRate 10-12, motor angles 17-28), d_est_out (baseVInWorldFrame 3-5, baseVelocityInBaseFrame 6-8,
 * footPositionsInBaseFrame 12-23, basePosition 36-38), d_rpy [3][n] (as qrgpu_pack_state_batch takes it), d_gait_out [24][n] (desiredLegState 8-11,
 * legState 12-15) and, for the contacts alone, d_gait_state (allowSwitchLegState 20-23; required with d_fe_in, else may be NULL).
 * Writes, each array may be NULL, other rows left alone:
 *   d_fe_in     6-8 basePosition; 9 yaw; 10-13 quat_wxyz; 14-25 foot positions in the world frame, invertRigidTransform(basePosition, baseOrientation,
 *               footPositionsInBaseFrame) (qrRobot::GetFootPositionsInWorldFrame, qr_robot.cpp:222-230); 38-41 the contacts
 *               MPCStanceLegController::Run reads (:212), which UpdateDesCommand's UpdateFRatio sets: (desiredLegState STANCE and
 *               allowSwitchLegState) or legState EARLY_CONTACT (qr_torque_stance_leg_controller.cpp:109-123), 1 or 0
 *   d_fh_in     21-32 footPositionsInBaseFrame; 33-36 quat_wxyz; 37-39 rpy; 40-42 baseVelocityInBaseFrame; 43-45 rpyRate
 *   d_swing_in  36-38 basePosition; 39-42 quat_wxyz; 43-45 baseVInWorldFrame; 46-57 motor angles
 *   d_est_in_next  rows 41-44: desiredLegState of this tick's gait, which the next estimator update reads.  Usually d_est_in itself: the rows written
 *               are not among the rows read, and a lane loads every row it reads before its first store.  No other two arrays may overlap. */
int  qrgpu_trot_inputs_batch(qrgpu_ctx *ctx, int n, const float *d_est_in, const float *d_est_out, const float *d_rpy, const float *d_gait_out,
                             const float *d_gait_state, float *d_fe_in, float *d_fh_in, float *d_swing_in, float *d_est_in_next);

/* qrgpu_mpc_command_batch: the motor command of the MPC mode -- MPCStanceLegController::GetAction's command (qr_mpc_stance_leg_controller.cpp:129-156)
 * merged with the swing command (qrRaibertSwingLegController::GetAction, qr_swing_leg_controller.cpp:419, :426-459) as
 * qrLocomotionController::GetAction merges them (qr_locomotion_controller.cpp:128-147).
 *   d_tau [12][n] of qrgpu_tick_batch; d_qdes [24][n] of qrgpu_swing_targets_batch (angles, velocities: a leg not recomputed this tick keeps its last
 *   targets there, as the map does); d_swing_in rows 0-3 (the legs that call computed); d_gait_out (desiredLegState 8-11, legState 12-15, curLegState
 *   16-19); d_gait_state (allowSwitchLegState 20-23)
 *   d_cmd_mem [1][n] int  bit l: leg l has an entry in swingJointAnglesVelocities.  reset 1 clears it for every robot (Reset(), :100), a stage-reset
 *                      binding's mask per robot; then the legs flagged in d_swing_in are added.
 *   d_motor_cmd [QRGPU_MOTOR_CMD_ROWS][n] = p[12], Kp[12], d[12], Kd[12], tua[12].  A leg with an entry whose flag of :450-452 holds (legState SWING or
 *                      USERDEFINED_SWING, or curLegState SWING while allowSwitchLegState is false): {q, kp, qd, kd, tua_s}; every other motor
 *                      {0, early_contact_abad_kp on the abad of an EARLY_CONTACT leg else 0, 0, stance_kd, tau}.
 * The torque epilogue, as read from qr_fsm_state_locomotion.cpp:140-157, qr_wbc_locomotion_controller.cpp:205-217 and qr_safety_checker.cpp:48-66: the
 * compensation is added to tua of every motor after GetAction, swing commands included; UpdateLegCMD then overwrites tua of the legs in contact_state
 * with the WBC's torque; the clip comes last.  qrgpu_tick_batch applies the context's epilogue to d_tau accordingly, so tau is taken as it comes.
 * tua_s of a swing command is 0 with desc->epilogue applied to it (QRGPU_EPILOGUE_HIP_COMP: -+0.9 on the abad; QRGPU_EPILOGUE_CLIP) -- this call does not
 * read the context's flags, the caller passes the ones it set -- except on a leg that is also in contact_state (the contacts of
 * qrgpu_trot_inputs_batch), where the WBC's overwrite leaves d_tau. */
struct qrgpu_mpc_command_desc {
    float kp[12], kd[12];             /* robot->GetMotorKps / GetMotorKdp, config/a1_sim: (100, 100, 100) / (1, 2, 2) per leg */
    float stance_kd;                  /* qr_mpc_stance_leg_controller.cpp:145, :149: 3.0 */
    float early_contact_abad_kp;      /* :145: 100.0 */
    int   epilogue;                   /* QRGPU_EPILOGUE_* bits as given to qrgpu_set_torque_epilogue: 0 */
};
typedef struct qrgpu_mpc_command_desc qrgpu_mpc_command_desc;
void qrgpu_mpc_command_desc_default(qrgpu_mpc_command_desc *d);
int  qrgpu_mpc_command_batch(qrgpu_ctx *ctx, int n, const qrgpu_mpc_command_desc *desc, int reset, const float *d_tau, const float *d_qdes,
                             const float *d_swing_in, const float *d_gait_out, const float *d_gait_state, int *d_cmd_mem, float *d_motor_cmd);

/* qrgpu_velocity_inputs_batch: the data-flow stage of the velocity mode -- the force-balance trot, LocomotionMode::VELOCITY_LOCOMOTION with
 * TorqueStanceLegController and the VELOCITY case of the swing controller (JOY_TROT: qr_fsm_state_locomotion.cpp:98-101,
 * qr_stance_leg_controller_interface.cpp:85-93).  What qrgpu_trot_inputs_batch and the memory of qrgpu_mpc_command_batch are to the MPC trot: the reads
 * the controllers make on qrRobot, qrStateDataFlow, the estimator and the gait generator between the stages, and the keys of
 * swingJointAnglesVelocities.  One launch on the context's stream, one lane per robot, workgroups of 64; copies, compares and integer bit operations.
 * The order of a tick: command update (d_swing_vel_in NULL), gait, this call, swing update (mode VELOCITY, given d_swing_vel_in: rows 8-19),
 * qrgpu_swing_velocity_batch, qrgpu_stance_tick_batch (mode VELOCITY, d_swing_q and d_swing_flag as below).
 * Reads d_est_in (quat_wxyz 6-9, yaw rate 12, motor angles 17-28), d_est_out (rows 6-8: stateEstimator->GetEstimatedVelocity(), which
 * qr_robot_velocity_estimator.cpp:126-131 leaves in the base frame -- the estimator kernel's baseVelocityInBaseFrame), d_ground_out (baseRInControlFrame
 * 22-30; read on terrain >= 2 alone, may be NULL below), d_gait_out [24][n] (normalizedPhase 4-7, desiredLegState 8-11, legState 12-15), d_gait_state
 * (allowSwitchLegState 20-23), d_state_des [12][n] of qrgpu_command_update_batch.  terrain: the TerrainType, 0..4 (PLANE, PLUM_PILES, STAIRS, SLOPE, ROUGH).
 * Writes, each of the four arrays may be NULL, no other row touched:
 *   d_swing_vel_in  0-3 the leg is in swingFootIds: not ((legState STANCE and allowSwitchLegState) or legState EARLY_CONTACT), 1 or 0
 *               (qr_swing_leg_controller.cpp:218-229); 4-7 normalizedPhase; 20-22 the estimated velocity; 23 GetBaseRollPitchYawRate()(2); 24-27 stateDes 6,
 *               7, 8, 11 -- the rows qr_swing_velocity_kernel reads, whatever qrgpu_command_update_batch or qrgpu_fsm_zero_command_batch put into rows
 *               23-26 before this call; 28-36 dR and 37-40 the quaternion of robotBaseR: the identity and (1, 0, 0, 0) on terrain < 2 (:271-276), else
 *               baseRInControlFrame and quat_wxyz; 41-52 motor angles.  Rows 8-19 (phaseSwitchFootLocalPos) are qrgpu_swing_update_batch's.
 *   d_est_in_next   rows 41-44: desiredLegState of this tick's gait, as qrgpu_trot_inputs_batch writes them.  Usually d_est_in itself: the rows written are
 *               not among the rows read, and a lane loads every row it reads before its first store.  No other two arrays may overlap.
 *   d_cmd_mem [1][n] int  bit l: leg l has an entry in swingJointAnglesVelocities.  reset 1 clears it for every robot (Reset(), :100), a stage-reset
 *               binding's mask per robot when the scalar is 0; then every leg of swingFootIds is added (GetAction, :408-424).  Required with d_swing_flag.
 *   d_swing_flag [4][n]  1 or 0: leg l has an entry and desiredLegState[l] == SWING (the VELOCITY case of the command loop, :446-448): the d_swing_flag of
 *               qrgpu_stance_command_batch / qrgpu_stance_tick_batch.
 * The values of the map are not kept by this call: they are rows 24-47 of qrgpu_swing_velocity_batch's d_out, which that kernel writes for the flagged
 * legs alone, so the array keeps a leg's last targets as the map does; d_swing_q of qrgpu_stance_command_batch is that d_out + 24 * n.
 * QRGPU_ERR_BAD_ARG, nothing launched, qrgpu_last_error naming the argument: n, terrain outside 0..4, reset other than 0 or 1, a NULL d_est_in, d_est_out,
 * d_gait_out, d_gait_state or d_state_des, a NULL d_ground_out on terrain >= 2, d_swing_flag without d_cmd_mem. */
int  qrgpu_velocity_inputs_batch(qrgpu_ctx *ctx, int n, int terrain, int reset, const float *d_est_in, const float *d_est_out, const float *d_ground_out,
                                 const float *d_gait_out, const float *d_gait_state, const float *d_state_des, float *d_swing_vel_in, float *d_est_in_next,
                                 int *d_cmd_mem, float *d_swing_flag);

/* ---- the control state machine: joystick, stand-up, transitions ---------------------------------------------------------------------------------
 * What decides when a robot is in qrFSMStateLocomotion::Run, per robot and per tick, with no host decision: qrDesiredStateCommand::JoyCallback and the
 * change-request block of Update (QS/controllers/qr_desired_state_command.cpp:66-161, :166-211), qrControlFSM::RunFSM over the states Passive, StandUp
 * and Locomotion (QS/fsm/ *.cpp, with SwitchMode, StandLoop and SafetyPostCheck) and Action::StandUp / SitDown (QS/action/qr_action.cpp:31-96).  Three
 * entry points, one launch each on the context's stream, one lane per robot; copies, compares, integer counters and float32 + - x / with contraction
 * off.  They change no other call.  The tick of a robot's whole life cycle (tools/closed_loop.py --fsm):
 *     episode step, qrgpu_fsm_update_batch, [plant,] observe ... qrgpu_command_update_batch, qrgpu_fsm_zero_command_batch, the locomotion chain ...
 *     qrgpu_mpc_command_batch (or qrgpu_stance_command_batch), qrgpu_fsm_command_batch.
 *
 * qrgpu_fsm_update_batch: everything qrRobotRunner::Update does before the locomotion chain.  Per robot, in this order:
 *   1. reset -- the scalar, or (d_done[r] & bits) != 0 -- writes the d_fsm_state column as constructed; what it held is not read: joyCtrlState =
 *      desc->initial_ctrl_state, prevJoyCtrlState JOY_STAND, movementMode 0, bodyUp 0, joyCtrlOnRequest 1, no request; the FSM in STAND_UP after its
 *      OnEnter (standUp 1, isUp 1, fsmMode K_STAND_UP), operating mode NORMAL; the locomotion state's checks on, the others' off; no command sent yet.
 *   2. JoyCallback, if a message arrived: d_joy_msg [QRGPU_JOY_MSG_ROWS][n] (may be NULL): row 0 != 0 "a message arrived this tick", rows 1-5 buttons
 *      [0] A, [1] B, [2] X, [3] Y, [5] RB (pressed: == 1), rows 6-8 axes [0], [3], [4], row 9 != 0 sets the gaitSwitch member (:166-169; read whatever row 0
 *      says).  Or from the device script d_script [QRGPU_FSM_SCRIPT_ROWS][n_script] (may be NULL): row 0 a tick count, row 1 a button mask
 *      (QRGPU_JOY_BTN_*), rows 2-4 axes [0], [3], [4]: a robot whose d_ticks[r] (row 0 of d_ep_state) equals an entry's tick receives that entry
 *      (the first such entry).  A row-0 message of d_joy_msg wins over the script.  The axes are scaled by desc->max_velx, max_vely, max_yawrate.
 *   3. unless an action is in progress: the gaitSwitch test and the change-request block of Update, and the zeros its JOY_STAND and else branches
 *      assign to the joyCmd members (:213-243);
 *   4. the head of RunFSM: a request becomes fsmMode (:72-94);
 *   5. CheckTransition of the current state and the operating-mode logic (:96-119), up to the decision of what runs this tick.
 *   d_joy [QRGPU_JOY_ROWS][n]  as qrgpu_command_update_batch reads it: rows 0-5 the joyCmd members (in HARD_CODE desc->hard_code_v, hard_code_w), 6
 *                      desc->body_height, 7 joyCtrlState.
 *   d_plan [n]         QRGPU_FSM_PLAN_* bits: exactly one of RUN (qrFSMStateLocomotion::Run), PHASE1 (SwitchMode / StandLoop: locomotion Update +
 *                      GetAction with the command zeroed), PHASE2 (SwitchMode's stand blend), ACTION (one tick of StandUp / SitDown), HOLD
 *                      (qrFSMStateStandUp::Run's command), PASSIVE (zeros), REPEAT (the command of the previous tick once more: see below); and the
 *                      flags DONE (transitionData.done: OnExit and OnEnter follow), ACTION_FIRST, ACTION_END.
 *   d_stage_mask [n] (may be NULL) = (d_done[r] & bits) | QRGPU_FSM_ENTERED where the robot's FSM ran qrFSMStateLocomotion::OnEnter with a state other
 *                      than HARD_CODE at the end of the previous tick (:88-124): bound with qrgpu_set_stage_reset (bits = the caller's |
 *                      QRGPU_FSM_ENTERED) it gives this tick's stages quadruped->Reset(), locomotionController->Reset() and stateEstimators->Reset().
 * qrgpu_fsm_zero_command_batch: stateDes.segment(6, 6) = 0 and UpdateControllerParams(..., 0, 0) of SwitchMode and StandLoop (:289-290, :329-330),
 *   after qrgpu_command_update_batch: for the robots whose plan has PHASE1, +0 into the copies of stateDes 6-11: d_state_des rows 6-11, d_fe_in 3-5,
 *   d_fh_in 16-19, d_swing_vel_in 23-26, d_stance_cmd 1-6.  Each array may be NULL; no other row, no other robot is touched.  Those are all the rows
 *   the existing kernels read desiredSpeed and desiredTwistingSpeed from; desired_speed / desired_twisting_speed of qrgpu_stance_desc are one value
 *   for the batch (user_parameters.yaml's, zero by default) and cannot be zeroed per robot.
 * qrgpu_fsm_command_batch: the rest of RunFSM, after the locomotion chain's motor command.  Reads d_plan, d_est_in (contacts 13-16, motor angles
 *   17-28) and d_motor_cmd_loco (what qrgpu_mpc_command_batch or qrgpu_stance_command_batch wrote; may be d_motor_cmd itself: a lane loads its column
 *   before its first store).  Writes every robot's d_motor_cmd [QRGPU_MOTOR_CMD_ROWS][n] column:
 *     RUN, PHASE1   the locomotion column passed through
 *     PHASE2        {stand ratio + (1 - ratio) q, Kp, 0, Kd, 0}, ratio = max(0.45f, (iter - T) / float(T))
 *     ACTION        {blend target + (1 - blend) q_before, Kp, 0, Kd, 0} (POSITION_MODE, qr_robot_a1_sim.cpp:676-684); blend = t / time; StandUp sends the
 *                   target itself once blend >= 1 (:48, :69); q_before is read from d_est_in at the action's first tick and kept in the state
 *     HOLD          {motorAngles, Kp, 0, Kd, 0}: the stand-up angles while isUp, else the sit-down angles
 *     PASSIVE       zeros
 *     REPEAT        the column this call wrote at the previous tick (kept in the state)
 *   then advances iter (with the N == 4 -> iter = T shortcuts), ends SwitchMode / StandLoop, runs OnExit and OnEnter after DONE and restores NORMAL, and
 *   clips the tua rows to +-desc->tau_clip while the current state's checkForceFeedForward is on (qr_safety_checker.cpp:48-66; idempotent on top of
 *   QRGPU_EPILOGUE_CLIP).  The reference's quirk is kept: Transition() to PASSIVE turns the locomotion state's checks off for good (:250).
 *   d_fsm_out [QRGPU_FSM_OUT_ROWS][n] (may be NULL), after the tick: 0 state name (FSM_StateName: PASSIVE 1, STAND_UP 4, LOCOMOTION 7), 1 operating mode
 *   (NORMAL 0, TRANSITIONING 1), 2 fsmMode, 3 joyCtrlState, 4 the locomotion state's iter, 5-7 checkSafeOrientation, checkPDesFoot,
 *   checkForceFeedForward of the current state, 8 the gait OnEnter chose last (QRGPU_FSM_GAIT_*; 0: none yet), 9 the mode (LocomotionMode; -1: none yet),
 *   10 action in progress (1 StandUp, -1 SitDown, 0).
 * d_fsm_state [QRGPU_FSM_STATE_ROWS][n] float32, the machine's memory, every integer held exactly (csrc/qr_fsm.h lists the rows).  The first call on
 *   new arrays is a reset.
 *
 * Unrolling, and what is OURS:
 *   - A blocking action becomes one ACTION tick per call.  Its loop variable t is kept in the state and advanced by t += time_step in float32 from a
 *     start time of 0 (the reference's wall-clock start is not reproducible).  The action ends at the first update call that finds t >= total
 *     (stand_up_total; sit_down_time): that call plans HOLD | ACTION_END, and the command call does what Run() does after the action.
 *   - While an action is in progress (that last call included) the runner is blocked: JoyCallback still runs; steps 3, 4 and 5 do not.
 *   - At most one joystick message per robot per tick.
 *   - fsmMode values that lead to statesList.invalid (BALANCE_STAND, VISION, RECOVERY_STAND, JOINT_PD) cannot arise from the joystick and are not
 *     supported: a state that meets one stays as it is.
 *   - PHASE1 passes the chain's command through as it comes: the batch tick cannot drop hip compensation and WBC for single robots.
 *   - REPEAT: where the reference sends a command kept from the tick before -- the tick that ends SwitchMode / StandLoop (transitionData.legCommand is
 *     not written, :276-283, :318-325), StandUp -> LOCOMOTION and LOCOMOTION -> STAND_UP (legCommand = data.legCmd) -- it is the column of the previous
 *     tick.  An empty legCommand (the transitions to and from PASSIVE, transitionData.Zero()) is written as zeros.
 *   - Gait and mode per robot are REPORTED in d_fsm_out.  qrgpu_gait_select_update_batch (below) acts on the gait, and qrgpu_mode_route_batch with
 *     qrgpu_set_mode_route and qrgpu_mode_command_batch (below) on the MODE, between the MPC chain and the force-balance chain.  The walk chain (with
 *     qrWalkGaitGenerator for the robots in JOY_WALK) and the position chain are not chosen per robot: such a robot falls back and is flagged.
 * QRGPU_ERR_BAD_ARG (nothing launched, outputs untouched; qrgpu_last_error names the argument): a NULL required array or desc; n < 1, n > max_batch;
 *   a reset other than 0 or 1; stand_up_time, stand_up_total, sit_down_time, time_step, a transition duration or tau_clip not finite or not > 0;
 *   transition_ticks < 1; initial_ctrl_state outside 0..7; n_script < 0 or > QRGPU_FSM_SCRIPT_MAX, n_script > 0 without d_script, a script without
 *   d_ticks; d_done with bits == 0. */
#define QRGPU_JOY_MSG_ROWS      10
#define QRGPU_FSM_SCRIPT_ROWS   5
#define QRGPU_FSM_SCRIPT_MAX    64
#define QRGPU_FSM_STATE_ROWS    106
#define QRGPU_FSM_OUT_ROWS      11
#define QRGPU_FSM_ENTERED       0x00010000  /* in d_stage_mask: outside QRGPU_EP_REASONS and QRGPU_EP_BAD_FIELD */
#define QRGPU_JOY_BTN_A         0x1         /* buttons[0] */
#define QRGPU_JOY_BTN_B         0x2         /* buttons[1] */
#define QRGPU_JOY_BTN_X         0x4         /* buttons[2] */
#define QRGPU_JOY_BTN_Y         0x8         /* buttons[3] */
#define QRGPU_JOY_BTN_RB        0x10        /* buttons[5] */
#define QRGPU_JOY_GAIT_SWITCH   0x20        /* the gaitSwitch member, not a button */
#define QRGPU_FSM_PLAN_RUN      0x1
#define QRGPU_FSM_PLAN_PHASE1   0x2
#define QRGPU_FSM_PLAN_PHASE2   0x4
#define QRGPU_FSM_PLAN_ACTION   0x8
#define QRGPU_FSM_PLAN_HOLD     0x10
#define QRGPU_FSM_PLAN_PASSIVE  0x20
#define QRGPU_FSM_PLAN_REPEAT   0x40
#define QRGPU_FSM_PLAN_DONE         0x100
#define QRGPU_FSM_PLAN_ACTION_FIRST 0x200
#define QRGPU_FSM_PLAN_ACTION_END   0x400
#define QRGPU_FSM_GAIT_TROT          1
#define QRGPU_FSM_GAIT_ADVANCED_TROT 2
#define QRGPU_FSM_GAIT_WALK          3
#define QRGPU_FSM_GAIT_STAND         4
struct qrgpu_fsm_desc {
    float stand_up_angles[12];        /* robot->standUpMotorAngles; a1_sim: (0, acos(0.28 / 2 / 0.2), -2 x that) per leg, in float (qr_robot_a1_sim.cpp:114-119) */
    float sit_down_angles[12];        /* robot->sitDownMotorAngles; a1_sim: (-0.167136, 0.934969, -2.54468) per leg */
    float kp[12], kd[12];             /* robot->motorKps / motorKds; a1_sim: 100 / (1, 2, 2) per leg */
    float stand_up_time;              /* qr_fsm_state_standup.cpp:62: 2 */
    float stand_up_total;             /* :62: 3 */
    float sit_down_time;              /* :66: 1.5 */
    float time_step;                  /* 1 / controlFrequency: 0.001 */
    int   transition_ticks;           /* T: every literal 1000 of SwitchMode, StandLoop and Transition */
    float gait_transition_duration;   /* qr_fsm_state_locomotion.cpp:176: 2 */
    float stand_transition_duration;  /* :181: 1 */
    float tau_clip;                   /* qr_safety_checker.cpp:57-60: 23 */
    float body_height;                /* robot->bodyHeight: 0.28 */
    int   initial_ctrl_state;         /* RC_MODE the command is constructed with (qr_desired_state_command.cpp:46): BODY_UP 5 */
    float hard_code_v[3], hard_code_w[3];                /* vDesInBodyFrame, wDesInBodyFrame: zeros */
    float max_velx, max_vely, max_yawrate;               /* the axes' scales, qr_desired_state_command.hpp:312, :322, :332: 0.2, 0.1, 0.2 */
};
typedef struct qrgpu_fsm_desc qrgpu_fsm_desc;
void qrgpu_fsm_desc_default(qrgpu_fsm_desc *d);
int  qrgpu_fsm_update_batch(qrgpu_ctx *ctx, int n, const qrgpu_fsm_desc *desc, int reset, const float *d_joy_msg /* may be NULL */,
                            const float *d_script /* [QRGPU_FSM_SCRIPT_ROWS][n_script], may be NULL */, int n_script, const int *d_ticks /* [n] */,
                            const int *d_done /* [n], may be NULL */, unsigned bits, float *d_fsm_state, float *d_joy, int *d_plan,
                            int *d_stage_mask /* may be NULL */);
int  qrgpu_fsm_zero_command_batch(qrgpu_ctx *ctx, int n, const int *d_plan, float *d_state_des, float *d_fe_in, float *d_fh_in,
                                  float *d_swing_vel_in, float *d_stance_cmd);
int  qrgpu_fsm_command_batch(qrgpu_ctx *ctx, int n, const qrgpu_fsm_desc *desc, const int *d_plan, const float *d_est_in,
                             const float *d_motor_cmd_loco, float *d_fsm_state, float *d_motor_cmd, float *d_fsm_out /* may be NULL */);

/* ---- the gait per robot: a table entry latched at reset, a clock that counts from OnEnter -----------------------------------------------------------
 * qrFSMStateLocomotion::OnEnter sets gaitGenerator->gait and calls locomotionController->Reset(); qrOpenLoopGaitGenerator::Reset
 * (QS/gait/qr_openloop_gait_generator.cpp:77-123) re-reads that gait's block of openloop_gait_generator.yaml, and qrLocomotionController::Reset
 * (QS/controllers/qr_locomotion_controller.cpp:56-66) restarts timeSinceReset.  Two entry points, one launch each on the context's stream, one lane per
 * robot; they change no other call.  The tick of tools/closed_loop.py --fsm-gait:
 *     episode step, qrgpu_fsm_update_batch, qrgpu_stage_clock_batch, qrgpu_set_stage_reset, plant, observe ... qrgpu_gait_select_update_batch ...
 *
 * qrgpu_gait_select_update_batch: qrgpu_gait_update_batch with the parameters of robot r taken from table[k_r], k_r chosen by the robot.
 *   table [n_gaits] (host; copied to the device when it differs from the table of the previous call), 1 <= n_gaits <= QRGPU_MAX_GAITS.
 *   d_gait_sel [n] float32: the integer index of robot r's gait in table; with the state machine row 44 of d_fsm_state (d_fsm_state + 44 * n), whose
 *     values are QRGPU_FSM_GAIT_*: 0 "none yet" is the gait the generator is constructed with.  It is read ONLY WHERE ROBOT r IS RESET AT THIS CALL -- the
 *     reference re-reads the parameters in Reset and nowhere else: changing `gait` between resets does nothing.  The index in force is kept in row 48 of
 *     d_gait_state and written back at every call; a call without a reset uses row 48, and a row 48 that does not hold an integer in [0, n_gaits) is
 *     read as 0.  A selection that is NaN, not an integer or outside [0, n_gaits) selects entry 0 and raises QRGPU_GAIT_BAD_SEL in d_gait_flags[r]
 *     (may be NULL).  That word is written at every call, 0 or the bit, never OR-ed; it is 0 where the selection was not read.
 *   Reset and clock are qrgpu_gait_update_batch's, per robot, whether or not a binding is set: the scalar `reset` (0, QRGPU_GAIT_RESET_CONSTRUCT,
 *     QRGPU_GAIT_RESET_LIVE) if it is non-zero; otherwise the bound level of qrgpu_set_stage_reset where (d_mask[r] & bits) != 0; otherwise none.  The
 *     clock is (float)d_ticks[r] * tick_dt of the binding when it has d_ticks, else current_time.
 *   A LIVE reset with a new entry is the reference's: the entry's initial_leg_state into the four leg-state vectors; resetTime, lastTime,
 *     normalizedPhase, contactStartPhase = 0; gaitCycle, cumDt, firstSwing, firstStance, swingTimeRemaining, phaseInFullCycle and allowSwitchLegState
 *     survive from the old gait (swingTimeRemaining keeps its last value for as long as the new gait commands no swing).  fullCyclePeriod,
 *     swingDuration, dutyFactor, contactDetectionPhaseThreshold, waitTime and the advanced-trot hold are the entry's from that call on.
 *   Rows 0-47 of d_gait_state, d_gait_out [24][n] (may be NULL) and rows 42-61 of d_fe_in (may be NULL) are written as qrgpu_gait_update_batch writes
 *     them, dutyFactor (46-49) of the robot's entry.  d_swing_in (may be NULL): rows 8-11 = swingDuration of the entry in force,
 *     stance_duration / duty_factor - stance_duration in float32 in that order, at every call; no other row of it.  Rows 49-51 of d_gait_state stay
 *     spare and are not written.
 *   QRGPU_ERR_BAD_ARG (nothing launched, outputs untouched; qrgpu_last_error names the argument): wherever qrgpu_gait_update_batch returns it; n_gaits
 *     < 1 or > QRGPU_MAX_GAITS; a NULL table or d_gait_sel; an entry with a duty factor <= 0.001 or a stance duration <= 0 (USERDEFINED_SWING legs are
 *     not supported).
 * qrgpu_gait_table_default: the five entries QRGPU_FSM_GAIT_* index, from config/a1_sim/openloop_gait_generator.yaml: [0] and [2] advanced_trot (each
 *   equal to qrgpu_gait_desc_default byte for byte), [1] trot (0.3, 0.6, phases (0.5, 0, 0, 0.5), threshold 0.5), [3] walk (7.5, 0.75, phases
 *   (0.5, 0, 0.75, 0.25), threshold 0.1: the walk block's parameters in the OPEN-LOOP generator, as OnEnter does it), [4] stand (0.3, duty 1, phases 0,
 *   threshold 0.1); advanced_trot = 0 in [1], [3], [4]; every entry starts its legs in STANCE and has qrgpu_gait_desc_default's wait_time.
 *
 * qrgpu_stage_clock_batch: where (d_mask[r] & bits) != 0, d_origin[r] = d_ticks[r]; then d_local[r] = d_ticks[r] - d_origin[r], in integers.  d_origin
 *   [n] is the clock's memory: at the first call on a new one every robot is masked, or it is zeroed.  With d_mask = the state machine's d_stage_mask,
 *   bits = QRGPU_EP_REASONS | QRGPU_FSM_ENTERED, d_ticks = row 0 of d_ep_state and d_local given to qrgpu_set_stage_reset as its d_ticks, every stage
 *   that reads the binding's clock -- the gait, the walk gait, the stance update and the stance tick -- counts from the robot's last OnEnter or spawn:
 *   resetTime = robot->GetTimeSinceReset().  No stage kernel changes for it.
 *   QRGPU_ERR_BAD_ARG: a NULL array, bits == 0, n < 1, n > max_batch. */
#define QRGPU_MAX_GAITS    8
#define QRGPU_GAIT_BAD_SEL 0x1
void qrgpu_gait_table_default(qrgpu_gait_desc table[5]);
int  qrgpu_gait_select_update_batch(qrgpu_ctx *ctx, int n, const qrgpu_gait_desc *table /* host, [n_gaits] */, int n_gaits,
                                    const float *d_gait_sel /* [n] */, float current_time, int robot_stop, int reset, const float *d_contact,
                                    float *d_gait_state, float *d_gait_out, float *d_fe_in, float *d_swing_in /* may be NULL */,
                                    int *d_gait_flags /* [n], may be NULL */);
int  qrgpu_stage_clock_batch(qrgpu_ctx *ctx, int n, const int *d_mask, unsigned bits, const int *d_ticks, int *d_origin /* [n], memory */,
                             int *d_local /* [n] */);

/* ---- the mode per robot: each robot's solve runs in the chain its state machine chose ----------------------------------------------------------------
 * qrFSMStateLocomotion::OnEnter sets the LocomotionMode with the gait (QS/fsm/qr_fsm_state_locomotion.cpp:78-158): JOY_TROT is VELOCITY_LOCOMOTION --
 * TorqueStanceLegController, the velocity case of the swing controller, the force-balance QP, no MPC and no WBC -- and JOY_ADVANCED_TROT is the MPC on
 * its cadence, the WBC and the hip compensation.  A robot that sits, stands up or holds runs no locomotion controller at all (:162-171).  Three things
 * are per robot here: which chain a robot is on (the route), the SOLVES of that chain (the binding), and whose motor command it gets (the merge).  The
 * cheap stage kernels -- one lane per robot, a few microseconds a launch -- still run on every robot in both chains; every one with memory takes the
 * stage-reset binding, so a robot entering a mode gets its Reset() calls through QRGPU_FSM_ENTERED in both chains' stages.  The caller keeps one set of
 * arrays per chain where the chains write different things (d_swing_state, d_swing_flags, d_cmd_mem, d_force, d_tau, d_status, d_motor_cmd); the
 * command, gait, ground, estimator and observe arrays are shared.  The tick of tools/closed_loop.py --fsm-mode:
 *     episode step, qrgpu_fsm_update_batch, qrgpu_stage_clock_batch, qrgpu_set_stage_reset, qrgpu_mode_route_batch, qrgpu_set_mode_route, plant, observe
 *     ... qrgpu_command_update_batch, qrgpu_fsm_zero_command_batch, qrgpu_gait_select_update_batch, the MPC chain up to qrgpu_mpc_command_batch, the
 *     force-balance chain up to qrgpu_stance_tick_batch, qrgpu_mode_command_batch, qrgpu_fsm_command_batch.
 *
 * qrgpu_mode_route_batch: one launch on the context's stream, one lane per robot, integer compares.
 *   desc->chain_of_mode[m] is the chain of LocomotionMode m (QRGPU_MODE_VELOCITY, _POSITION, _WALK, _ADVANCED_TROT), desc->fallback_chain the chain of a
 *     robot whose mode has none.  qrgpu_mode_route_desc_default: {FORCE_BALANCE, NONE, NONE, MPC}, fallback MPC.
 *   d_mode_sel [n] float32, like d_gait_sel: with the state machine row 45 of d_fsm_state (d_fsm_state + 45 * n).  It is read at EVERY call: the machine
 *     latches it at OnEnter, so there is nothing left to latch here.
 *   d_plan [n] (may be NULL): the state machine's plan of this tick.
 *   d_chain [n], per robot, in this order:
 *     d_plan is given and has neither QRGPU_FSM_PLAN_RUN nor QRGPU_FSM_PLAN_PHASE1        QRGPU_CHAIN_NONE, flags 0
 *     mode -1 ("none yet")                                                                 QRGPU_CHAIN_NONE, flags 0
 *     mode NaN, not an integer, or outside -1..3                                           fallback_chain, QRGPU_ROUTE_BAD_MODE
 *     chain_of_mode[mode] == QRGPU_CHAIN_NONE                                              fallback_chain, QRGPU_ROUTE_NO_CHAIN
 *     otherwise                                                                            chain_of_mode[mode], flags 0
 *     With the defaults POSITION and WALK take the fourth line: those chains are not closed on the device, so such a robot runs on the MPC chain and is
 *     flagged -- the rule of the gait table, where the walk parameters run in the open-loop generator: run something and say so.
 *     Mode -1 is what the machine reports until an OnEnter under JOY_TROT, JOY_ADVANCED_TROT or JOY_WALK has set one; the reference's robot then
 *     still runs the mode its controller was CONSTRUCTED with, which the machine does not know.  So a robot whose first OnEnter comes under JOY_STAND
 *     (the "MPC standing" phase of tools/closed_loop.py --fsm) is on no chain and gets zeros until its first gait button: a caller who wants such
 *     robots held up hands this call a d_mode_sel of its own with the constructed mode in place of -1.  Open.
 *   d_route_flags [n] (may be NULL) is written at every call, 0 or one bit, never OR-ed.
 *   d_chain_count [3] (may be NULL): d_chain_count[c] = the number of robots on chain c.  The call zeroes it on the stream; the kernel adds one integer
 *     per chain and wavefront (ballot, popcount, atomicAdd): the sums do not depend on the order.
 *   QRGPU_ERR_BAD_ARG (nothing launched, outputs untouched; qrgpu_last_error names the argument): a NULL desc, d_mode_sel or d_chain; n < 1, n >
 *     max_batch; a table entry or the fallback outside 0..2.
 *
 * qrgpu_set_mode_route: binds d_chain [n] (NULL: off).  The pointer is copied into the context and the array is read when the kernels run, exactly like
 *   qrgpu_set_stage_reset's mask.  While it is set:
 *   qrgpu_tick_cadence_batch: a robot with d_chain[r] != QRGPU_CHAIN_MPC is idle: the MPC launch, the cadence kernel and the WBC launch read and write
 *     nothing of it, and its columns of d_force, d_hold, d_tau, d_qdes, d_status and d_prev_ori stay as they were.  A robot on the MPC chain is handled
 *     exactly as without the binding.  (One launch more in front: due' = d_mpc_updated && on the chain for the MPC launch, skip' = d_mpc_updated || not
 *     on the chain for the WBC launch, in two arrays of the context.  A batch with nobody on the MPC chain still makes every launch; each ends at once.)
 *   qrgpu_stance_tick_batch, qrgpu_vmc_force_batch, qrgpu_vmc_force_world_batch: the force-balance QP's workgroup of a robot with d_chain[r] !=
 *     QRGPU_CHAIN_FORCE_BALANCE returns before its first load: the robot's d_force, d_tau and d_status columns stay as they were.  The update and
 *     command kernels of the stance tick still run for every robot, so an idle robot's d_motor_cmd column IN THE FORCE-BALANCE CHAIN'S ARRAY is made
 *     from a stale d_tau; nothing selects it.
 *   EVERY OTHER ENTRY POINT IGNORES THE BINDING: qrgpu_tick_batch in its serial, pipelined and overlapped forms (they rest on every robot's solve raising
 *     a flag), qrgpu_mpc_solve_batch, qrgpu_wbc_run_batch, the single-robot calls (qrgpu_mpc_solve1, qrgpu_wbc_run1, qrgpu_vmc_force1,
 *     qrgpu_vmc_force_world1), the debug and inspection calls (qrgpu_mpc_assemble_batch, qrgpu_fb_debug_batch, qrgpu_wbc_inspect_batch), and every stage kernel (gait, swing, foothold, front-end, stance update and command, estimator, ground, observe, command, data
 *     flow, state machine, plant, episode).
 *   What a robot that changes chains carries over: nothing on the force-balance side (the QP has no memory; the stages are reset by
 *     QRGPU_FSM_ENTERED).  On the MPC side the front-end's reset (MPCStanceLegController::Reset, qr_mpc_stance_leg_controller.cpp:78-92:
 *     iterationCounter = 0) makes the tick of OnEnter and the 49 that follow due ones (UpdateMPC re-plans on each of the first 50 ticks), so d_hold is
 *     rewritten before it is read and the WBC, which alone reads d_prev_ori, first runs again 50 ticks later.  It then finds what the robot's last WBC
 *     pass left there, however long ago: the reference's wbcController is made once with the locomotion state (qr_fsm_state_locomotion.cpp:61) and no
 *     OnEnter resets it.  The warm-start words of the robot's last solve stay too (speed only).
 *
 * qrgpu_mode_command_batch: one launch, one lane per robot.  Robot r's d_motor_cmd [QRGPU_MOTOR_CMD_ROWS][n] column and d_status word (may be NULL) are
 *   those of its chain: d_cmd_mpc and d_status_mpc (may be NULL: 0) where d_chain[r] == QRGPU_CHAIN_MPC, d_cmd_fb and d_status_fb (may be NULL: 0) where
 *   it is QRGPU_CHAIN_FORCE_BALANCE; QRGPU_CHAIN_NONE, or any value outside 1..2, gives zeros and status 0.  The copy is bit for bit and a select, not a
 *   blend: a NaN in the column that is not selected never reaches the output.  d_motor_cmd may be either input, d_status either status input (a lane
 *   loads both columns before its first store, as in qrgpu_fsm_command_batch), which follows and reads d_motor_cmd as its d_motor_cmd_loco.
 *   QRGPU_ERR_BAD_ARG (nothing launched; qrgpu_last_error names the argument): a NULL d_chain, d_cmd_mpc, d_cmd_fb or d_motor_cmd; n < 1, n > max_batch. */
#define QRGPU_CHAIN_NONE           0
#define QRGPU_CHAIN_MPC            1
#define QRGPU_CHAIN_FORCE_BALANCE  2
#define QRGPU_ROUTE_BAD_MODE  0x1
#define QRGPU_ROUTE_NO_CHAIN  0x2
struct qrgpu_mode_route_desc {
    int chain_of_mode[4];             /* QRGPU_CHAIN_* per LocomotionMode (QRGPU_MODE_*) */
    int fallback_chain;               /* the chain of a robot whose mode has none, or is not a mode */
};
typedef struct qrgpu_mode_route_desc qrgpu_mode_route_desc;
void qrgpu_mode_route_desc_default(qrgpu_mode_route_desc *d);
int  qrgpu_mode_route_batch(qrgpu_ctx *ctx, int n, const qrgpu_mode_route_desc *desc, const float *d_mode_sel /* [n] */,
                            const int *d_plan /* [n], may be NULL */, int *d_chain /* [n] */, int *d_route_flags /* [n], may be NULL */,
                            int *d_chain_count /* [3], may be NULL */);
int  qrgpu_set_mode_route(qrgpu_ctx *ctx, const int *d_chain /* NULL: off */);
int  qrgpu_mode_command_batch(qrgpu_ctx *ctx, int n, const int *d_chain, const float *d_cmd_mpc,
                              const float *d_cmd_fb /* [QRGPU_MOTOR_CMD_ROWS][n] each */, const int *d_status_mpc,
                              const int *d_status_fb /* may be NULL */, float *d_motor_cmd, int *d_status /* may be NULL */);

/* ---- multi-GPU: all-gather of the per-robot torques over RCCL / xGMI ----------------------------------------
 * One process per GPU, one context per process; rank r of N owns a contiguous shard of the robot population and there is no exchange
 * inside a tick.  The only collective of the path collects every rank's tau[12][n_local] on every rank:
 *     d_tau_all [nranks][12][n_local]   (rank-major; block r is rank r's d_tau)
 * The communicator is created from a 128-byte id blob (ncclUniqueId) that rank 0 makes and the launcher hands to the other ranks by
 * whatever channel it has (MPI, a file, torch.distributed's CPU backend ...): no collective library appears in this ABI's signatures.
 * qrgpu_allgather_tau takes either that context-owned communicator (nccl_comm = NULL) or the caller's own ncclComm_t.  It is asynchronous:
 * the gather waits for the work queued on the context's compute stream so far, runs on a stream of the context's own, and the next
 * tick may be issued at once.  `slot` (0 / 1) names the torque buffer being read for double buffering: call qrgpu_allgather_fence(slot)
 * before queueing work that overwrites that buffer, qrgpu_comm_sync to wait on the host for every gather issued so far.
 * A consumer of d_tau_all queued on the context's compute stream waits for the gather with qrgpu_allgather_wait(slot) (a stream-side wait,
 * no host block; it leaves the fence of that slot due).  The gather of tick i + 1 starts as soon as tick i + 1's torques are complete: a
 * consumer of tick i's d_tau_all that is queued AFTER qrgpu_allgather_tau of tick i + 1 would race with it, so either queue the consumer
 * first or give d_tau_all two buffers by slot as well. */
#define QRGPU_COMM_ID_BYTES 128
int qrgpu_comm_unique_id(unsigned char id[QRGPU_COMM_ID_BYTES]);
int qrgpu_comm_init_rank(qrgpu_ctx *ctx, const unsigned char id[QRGPU_COMM_ID_BYTES], int nranks, int rank);
int qrgpu_comm_info(const qrgpu_ctx *ctx, int *nranks, int *rank);
int qrgpu_comm_destroy(qrgpu_ctx *ctx);
int qrgpu_allgather_tau(qrgpu_ctx *ctx, void *nccl_comm /* ncclComm_t, or NULL = the context's */, const float *d_tau /* [12][n_local] */,
                        int n_local, float *d_tau_all /* [nranks][12][n_local] */, int slot);
/* The same for the torque array that the context's most recent qrgpu_tick_batch produced, when nothing the caller has queued on the context's
 * stream since writes it: the gather then waits for THAT TICK to be complete (its join bumps a count the communication stream polls) instead of for
 * an event of the context's stream -- recording one costs that stream several microseconds a tick.  Falls back to qrgpu_allgather_tau's form when
 * the last tick was not a pipelined one (fewer than 64 robots, qrgpu_set_tick_pipeline off, a stream under graph capture). */
int qrgpu_allgather_tau_of_tick(qrgpu_ctx *ctx, void *nccl_comm, const float *d_tau, int n_local, float *d_tau_all, int slot);
int qrgpu_allgather_fence(qrgpu_ctx *ctx, int slot);
int qrgpu_allgather_wait(qrgpu_ctx *ctx, int slot);
int qrgpu_comm_sync(qrgpu_ctx *ctx);

/* ---- single-robot host-pointer API (what the drop-in C++ adapters call) ------ */
int qrgpu_mpc_solve1(qrgpu_ctx *ctx, int type_id, const float p[3], const float v[3], const float quat_wxyz[4],
                     const float w[3], const float r_3x4_colmajor[12], const float rpy[3],
                     const float *traj /*12h*/, const float *gait /*4h*/, const float q[12] /*may be NULL*/,
                     double f_out[12], float tau_out[12] /*may be NULL*/, int *status);
int qrgpu_wbc_run1(qrgpu_ctx *ctx, int type_id, const float fb_state[37], const float wbc_cmd[67],
                   float prev_ori_vel[3], float tau_out[12], float qdes_out[12], float qddes_out[12], int *status);

int qrgpu_vmc_force1(qrgpu_ctx *ctx, int type_id, const float vmc_in[37], const float q[12] /*may be NULL*/,
                     float force_out[12], float tau_out[12] /*may be NULL*/, int *status);
int qrgpu_vmc_force_world1(qrgpu_ctx *ctx, int type_id, const float vmc_in[37], const float ratio[8] /* fMinRatio[4], fMaxRatio[4] */,
                           const float q[12] /*may be NULL*/, float force_out[12], float tau_out[12] /*may be NULL*/, int *status);

/* ---- inspection (parity tests): the fp32 QP data the MPC kernel assembled ----- */
/* d_H: [n][12h*12h] row-major per robot, d_g: [n][12h]; entries that involve a swing
 * (eliminated) variable are left untouched. */
int qrgpu_mpc_assemble_batch(qrgpu_ctx *ctx, int n, const int *d_type_id, const float *d_mpc_state,
                             const float *d_traj, const float *d_gait, float *d_H, float *d_g);
/* Rigid-body quantities the WBC kernel computed: d_out [n][QRGPU_FB_DEBUG_FLOATS]
 * = H(324) G(18) C(18) Jc(4*54) Jcdqd(12) pGC(12) vGC(12). */
#define QRGPU_FB_DEBUG_FLOATS (324 + 18 + 18 + 216 + 12 + 12 + 12)
int qrgpu_fb_debug_batch(qrgpu_ctx *ctx, int n, const int *d_type_id, const float *d_fb_state, float *d_out);

/* One WBC tick as qrgpu_wbc_run_batch computes it (K12 skipped), plus the solution of its relaxation QP:
 * d_qp [n][QRGPU_WBC_QP_FLOATS] = qpz[18] (z_fb[6], z_f[3 * contacts], zero padded; qr_wholebody_impulse_ctrl.cpp:113) and
 * extraData->optimalFr[12] = z_f + Fr_des (:216-218), stance feet in contact order, zero padded. */
#define QRGPU_WBC_QP_FLOATS 30
int qrgpu_wbc_inspect_batch(qrgpu_ctx *ctx, int n, const int *d_type_id, const float *d_fb_state, const float *d_wbc_cmd,
                            float *d_prev_ori, float *d_tau, float *d_qp, int *d_status);

/* ---- executed arithmetic of the batched MPC solve (measurement; off by default) ---------------------------------------------------
 * With counting on, every solve leaves what it actually computed, by formula from the sizes it saw (stance leg-steps, tile count,
 * working-set size of every change, rebuilds): out[0] fp32 vector flops, out[1] fp32 matrix flops issued (v_mfma_f32_16x16x4_f32),
 * out[2] fp64 flops of the block sweep and x0, out[3] fp64 flops of the active set.  qrgpu_mpc_flop_counts sums them over the robots of
 * the last counted call (mul and add count 1, fma 2).  bench.py's roofline block is built from these, not from a dense yardstick. */
int qrgpu_enable_flop_count(qrgpu_ctx *ctx, int on);
int qrgpu_mpc_flop_counts(qrgpu_ctx *ctx, double out[4]);

/* ---- plumbing ------------------------------------------------------------------ */
int  qrgpu_sync(qrgpu_ctx *ctx);                       /* hipStreamSynchronize on the context stream */
/* Mean device time (ms) of the kernels launched by the last `calls` batched calls,
 * measured with hipEvents on the context stream; kernel: 0 = MPC, 1 = WBC.
 * on = 0: off; 1: events around every launch; N > 1: around every N-th launch of a kernel (an event
 * pair costs a 0.3 ms tick about 4 us per kernel; the mean is over the bracketed launches);
 * -1: pause (the next on > 0 carries on with what was measured so far; on = 0 forgets it). */
int  qrgpu_enable_timing(qrgpu_ctx *ctx, int on);
int  qrgpu_get_timing(qrgpu_ctx *ctx, int kernel, double *mean_ms, int *count);
void *qrgpu_malloc(qrgpu_ctx *ctx, unsigned long long bytes);   /* hipMalloc on the context device */
void qrgpu_free(qrgpu_ctx *ctx, void *p);
int  qrgpu_memcpy_h2d(qrgpu_ctx *ctx, void *dst, const void *src, unsigned long long bytes);
int  qrgpu_memcpy_d2h(qrgpu_ctx *ctx, void *dst, const void *src, unsigned long long bytes);
/* Pinned host memory and asynchronous copies on the context stream (kind: 0 host->device, 1 device->host, 2 device->device; the host
 * side should be qrgpu_host_alloc memory), an asynchronous byte fill, and caller-indexed timing marks: qrgpu_mark(i) records event i on
 * the context stream (index < 65536; created on first use), qrgpu_mark_elapsed_ms waits for mark `to` and returns the device time between
 * the two.  Launcher plumbing for callers that use no GPU array library (bench.py). */
void *qrgpu_host_alloc(qrgpu_ctx *ctx, unsigned long long bytes);
void qrgpu_host_free(qrgpu_ctx *ctx, void *p);
int  qrgpu_memcpy_async(qrgpu_ctx *ctx, void *dst, const void *src, unsigned long long bytes, int kind);
int  qrgpu_memset_async(qrgpu_ctx *ctx, void *dst, int byte_value, unsigned long long bytes);
int  qrgpu_mark(qrgpu_ctx *ctx, int index);
int  qrgpu_mark_elapsed_ms(qrgpu_ctx *ctx, int from, int to, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* QRGPU_H */
