// The control state machine, per robot: what qr_fsm_update_kernel, qr_fsm_zero_kernel and qr_fsm_command_kernel (qr_fsm_kernel.hip) run per lane.
// Copies, compares, integer counters and float32 + - x / with contraction off.  Every function is __host__ __device__: the same text compiles for a CPU
// check against tests/fsm_ref.py (tests/stubs/fsm_host.hip).  include/qrgpu.h states the rules, the unrolling of the blocking actions and what is OURS.
//   qrDesiredStateCommand::JoyCallback, Update      quadruped/src/controllers/qr_desired_state_command.cpp:66-161, :166-243
//   qrControlFSM::Initialize, RunFSM, SafetyPostCheck   quadruped/src/fsm/qr_control_fsm.cpp:57-64, :68-152, :164-177
//   qrFSMStatePassive, qrFSMStateStandUp            quadruped/src/fsm/qr_fsm_state_passive.cpp, qr_fsm_state_standup.cpp
//   qrFSMStateLocomotion (SwitchMode, StandLoop)    quadruped/src/fsm/qr_fsm_state_locomotion.cpp:78-126, :162-355
//   qrSafetyChecker::CheckForceFeedForward          quadruped/src/fsm/qr_safety_checker.cpp:48-66
//   Action::StandUp, SitDown                        quadruped/src/action/qr_action.cpp:31-96
// Row k of an array lies at p[k * S]: the kernel passes the robot's column and S = n, a packed record has S = 1.
//
// d_fsm_state rows (float32, every integer exact):
//    0 joyCtrlState   1 prevJoyCtrlState   2 movementMode   3 bodyUp   4 joyCtrlOnRequest   5 joyCtrlStateChangeRequest   6 joyCmdExit   7 gaitSwitch
//    8-13 joyCmdVx, Vy, Vz, RollRate, PitchRate, YawRate
//   14 fsmMode   15 currentState (FSM_StateName)   16 operatingMode   17 nextState
//   18-22 locomotion state: nextStateName, transitionDuration, iter, its checks (on / off), transitionData.done
//   23-26 stand-up state: nextStateName, standUp, isUp, transitionData.done        27-28 passive state: nextStateName, transitionData.done
//   29 action in progress (1 StandUp, -1 SitDown)   30 its t   31-42 the motor angles before it
//   43 OnEnter of the locomotion state ran at the end of the tick (QRGPU_FSM_ENTERED of the next)   44 the gait it chose   45 the mode
//   46-105 the motor command of the previous tick
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/qrgpu.h"

#ifndef QR_HD
#define QR_HD __host__ __device__ __forceinline__
#endif

namespace qrgpu {
namespace fsm {

enum { RC_HARD_CODE = 0, RC_JOY_TROT, RC_JOY_ADVANCED_TROT, RC_JOY_WALK, RC_JOY_STAND, RC_BODY_UP, RC_BODY_DOWN, RC_EXIT };      // config/qr_enum_types.h:101-113
enum { K_STAND_DOWN = -1, K_PASSIVE = 0, K_STAND_UP = 1, GAIT_TRANSITION = 3, K_LOCOMOTION = 4, LOCOMOTION_STAND = 7 };        // fsm/qr_fsm_state.hpp:38-48
enum { ST_PASSIVE = 1, ST_STAND_UP = 4, ST_LOCOMOTION = 7 };                                                                  // FSM_StateName, :63-71
enum { OP_NORMAL = 0, OP_TRANSITIONING = 1 };                                                                                 // fsm/qr_control_fsm.hpp:40-45
enum { MODE_VELOCITY = 0, MODE_WALK = 2, MODE_ADVANCED_TROT = 3 };                                                            // LocomotionMode, :79-84
enum { S_CTRL = 0, S_PREV, S_MOVE, S_BODYUP, S_JOYON, S_REQ, S_EXIT, S_GAITSW, S_CMD, S_FSMMODE = 14, S_STATE, S_OP, S_NEXT, S_L_NEXT, S_L_DUR, S_L_ITER,
       S_L_CHECKS, S_L_DONE, S_SU_NEXT, S_SU_STANDUP, S_SU_ISUP, S_SU_DONE, S_P_NEXT, S_P_DONE, S_ACT, S_ACT_T, S_QBEFORE, S_ENTERED = 43, S_GAIT, S_MODE,
       S_LAST, S_ROWS = S_LAST + QRGPU_MOTOR_CMD_ROWS };
static_assert(S_ROWS == QRGPU_FSM_STATE_ROWS, "d_fsm_state rows");
enum { PLAN_KINDS = 0x7f };

// The scalar rows 0-45 of a column in registers: integers as int, the four float members as they are.
struct Machine {
    int ctrl, prev, move, body_up, joy_on, req, exit, gait_sw;
    float cmd[6];
    int fsm_mode, state, op, next, l_next;
    float l_dur;
    int l_iter, l_checks, l_done, su_next, stand_up, is_up, su_done, p_next, p_done, act;
    float act_t, qb[12];
    int entered, gait, mode;
};

// As constructed: qrDesiredStateCommand's constructor (:46-58), the three states' constructors, qrControlFSM::Initialize
QR_HD void construct(const qrgpu_fsm_desc &D, Machine &m)
{
    m.ctrl = D.initial_ctrl_state; m.prev = RC_JOY_STAND; m.move = 0; m.body_up = 0; m.joy_on = 1; m.req = 0; m.exit = 0; m.gait_sw = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) m.cmd[k] = 0.f;
    m.state = ST_STAND_UP; m.op = OP_NORMAL; m.next = ST_STAND_UP;
    m.l_next = ST_LOCOMOTION; m.l_dur = 0.f; m.l_iter = 0; m.l_checks = 1; m.l_done = 0;         // qrFSMStateLocomotion is constructed, not entered
    m.su_next = ST_STAND_UP; m.stand_up = 1; m.is_up = 1; m.su_done = 0; m.fsm_mode = K_STAND_UP;  // qrFSMStateStandUp::OnEnter
    m.p_next = ST_PASSIVE; m.p_done = 0;
    m.act = 0; m.act_t = 0.f;
#pragma unroll
    for (int k = 0; k < 12; ++k) m.qb[k] = 0.f;
    m.entered = 0; m.gait = 0; m.mode = -1;
}

// rst: the column is not decoded (a float that holds no integer is never cast)
QR_HD void load(const qrgpu_fsm_desc &D, bool rst, size_t S, const float *st, Machine &m)
{
    float s[S_LAST];
#pragma unroll
    for (int k = 0; k < S_LAST; ++k) s[k] = st[(size_t)k * S];
    if (rst) { construct(D, m); return; }
    m.ctrl = (int)s[S_CTRL]; m.prev = (int)s[S_PREV]; m.move = (int)s[S_MOVE]; m.body_up = (int)s[S_BODYUP]; m.joy_on = (int)s[S_JOYON]; m.req = (int)s[S_REQ];
    m.exit = (int)s[S_EXIT]; m.gait_sw = (int)s[S_GAITSW];
#pragma unroll
    for (int k = 0; k < 6; ++k) m.cmd[k] = s[S_CMD + k];
    m.fsm_mode = (int)s[S_FSMMODE]; m.state = (int)s[S_STATE]; m.op = (int)s[S_OP]; m.next = (int)s[S_NEXT];
    m.l_next = (int)s[S_L_NEXT]; m.l_dur = s[S_L_DUR]; m.l_iter = (int)s[S_L_ITER]; m.l_checks = (int)s[S_L_CHECKS]; m.l_done = (int)s[S_L_DONE];
    m.su_next = (int)s[S_SU_NEXT]; m.stand_up = (int)s[S_SU_STANDUP]; m.is_up = (int)s[S_SU_ISUP]; m.su_done = (int)s[S_SU_DONE];
    m.p_next = (int)s[S_P_NEXT]; m.p_done = (int)s[S_P_DONE];
    m.act = (int)s[S_ACT]; m.act_t = s[S_ACT_T];
#pragma unroll
    for (int k = 0; k < 12; ++k) m.qb[k] = s[S_QBEFORE + k];
    m.entered = (int)s[S_ENTERED]; m.gait = (int)s[S_GAIT]; m.mode = (int)s[S_MODE];
}

QR_HD void store(size_t S, const Machine &m, float *__restrict__ st)
{
    float s[S_LAST];
    s[S_CTRL] = (float)m.ctrl; s[S_PREV] = (float)m.prev; s[S_MOVE] = (float)m.move; s[S_BODYUP] = (float)m.body_up; s[S_JOYON] = (float)m.joy_on;
    s[S_REQ] = (float)m.req; s[S_EXIT] = (float)m.exit; s[S_GAITSW] = (float)m.gait_sw;
#pragma unroll
    for (int k = 0; k < 6; ++k) s[S_CMD + k] = m.cmd[k];
    s[S_FSMMODE] = (float)m.fsm_mode; s[S_STATE] = (float)m.state; s[S_OP] = (float)m.op; s[S_NEXT] = (float)m.next;
    s[S_L_NEXT] = (float)m.l_next; s[S_L_DUR] = m.l_dur; s[S_L_ITER] = (float)m.l_iter; s[S_L_CHECKS] = (float)m.l_checks; s[S_L_DONE] = (float)m.l_done;
    s[S_SU_NEXT] = (float)m.su_next; s[S_SU_STANDUP] = (float)m.stand_up; s[S_SU_ISUP] = (float)m.is_up; s[S_SU_DONE] = (float)m.su_done;
    s[S_P_NEXT] = (float)m.p_next; s[S_P_DONE] = (float)m.p_done;
    s[S_ACT] = (float)m.act; s[S_ACT_T] = m.act_t;
#pragma unroll
    for (int k = 0; k < 12; ++k) s[S_QBEFORE + k] = m.qb[k];
    s[S_ENTERED] = (float)m.entered; s[S_GAIT] = (float)m.gait; s[S_MODE] = (float)m.mode;
#pragma unroll
    for (int k = 0; k < S_LAST; ++k) st[(size_t)k * S] = s[k];
}

// ---- qrDesiredStateCommand::JoyCallback (:66-161).  btn: QRGPU_JOY_BTN_* bits; ax: axes [0], [3], [4]
QR_HD void joy_callback(const qrgpu_fsm_desc &D, int btn, const float ax[3], Machine &m)
{
#pragma clang fp contract(off)
    m.cmd[2] = 0.f;                                                              // joyCmdVz (:68)
    if (btn & QRGPU_JOY_BTN_A) m.joy_on = !m.joy_on;                             // :73-81
    // rosCmdRequest = !joyCtrlOnRequest: one of the two holds (:83-85)
    if (btn & QRGPU_JOY_BTN_X) {                                                 // :87-93
        if (m.move == 0) m.move = 1;
        m.req = 1;
    }
    if (m.joy_on) {                                                              // :96-117
        m.cmd[0] = ax[2] * D.max_velx;
        m.cmd[1] = ax[1] * D.max_vely;
        m.cmd[5] = ax[0] * D.max_yawrate;
        m.cmd[3] = 0.f;
        m.cmd[4] = 0.f;
    }
    if (btn & QRGPU_JOY_BTN_B) {                                                 // :120-132
        if (m.move == 1) {
            m.move = 0; m.req = 1;
        } else if (m.move == 0) {
            if (m.body_up >= 0) { m.body_up = 0; m.req = 1; }
        }
    }
    if (btn & QRGPU_JOY_BTN_Y) {                                                 // :137-144
        if (m.move == 0 && m.body_up <= 0) { m.exit = 1; m.req = 1; m.joy_on = 0; }
    }
    if (btn & QRGPU_JOY_BTN_RB) {                                                // :149-159
        if (m.move == 0) {
            m.body_up = m.body_up == 0 ? 1 : -m.body_up;
            m.req = 1;
        }
    }
}

// ---- the head of qrDesiredStateCommand::Update: gaitSwitch (:166-169), the change-request block (:173-211), the joyCmd zeros of :213-243
QR_HD void command_request(Machine &m)
{
    if (m.gait_sw) { m.req = 1; m.gait_sw = 0; }
    if (m.req) {
        if (m.move > 0) {
            if (m.ctrl == RC_HARD_CODE || m.ctrl == RC_BODY_UP) {
                m.ctrl = RC_JOY_STAND;
            } else if (m.ctrl == RC_JOY_STAND) {
                m.ctrl = RC_JOY_ADVANCED_TROT;
            } else {
                m.ctrl = (m.ctrl + 1) % (RC_EXIT + 1);
                if (m.ctrl == RC_HARD_CODE) m.ctrl = m.ctrl + 1;
                else if (m.ctrl > RC_JOY_ADVANCED_TROT) m.ctrl = RC_JOY_TROT;
            }
        } else {
            if (m.ctrl <= 3) m.prev = m.ctrl;
            if (m.exit) m.ctrl = RC_EXIT;
            else if (m.body_up == -1) m.ctrl = RC_BODY_DOWN;
            else if (m.body_up == 1) m.ctrl = RC_BODY_UP;
            else m.ctrl = RC_JOY_STAND;
        }
    }
    if (!(m.ctrl == RC_JOY_TROT || m.ctrl == RC_JOY_ADVANCED_TROT || m.ctrl == RC_JOY_WALK || m.ctrl == RC_HARD_CODE)) {
#pragma unroll
        for (int k = 0; k < 6; ++k) m.cmd[k] = 0.f;
    }
}

// ---- SwitchMode / StandLoop as far as iter decides: what the tick sends (:276, :287, :318, :328)
QR_HD int self_transition_plan(const qrgpu_fsm_desc &D, const Machine &m)
{
#pragma clang fp contract(off)
    const int T = D.transition_ticks;
    const float span = m.l_dur * (float)T;
    if (m.fsm_mode == GAIT_TRANSITION) {
        if ((float)m.l_iter >= span) return QRGPU_FSM_PLAN_REPEAT | QRGPU_FSM_PLAN_DONE;
        return m.l_iter < T ? QRGPU_FSM_PLAN_PHASE1 : QRGPU_FSM_PLAN_PHASE2;
    }
    if (m.l_iter >= T) return QRGPU_FSM_PLAN_REPEAT | QRGPU_FSM_PLAN_DONE;
    return (float)m.l_iter < span ? QRGPU_FSM_PLAN_PHASE1 : QRGPU_FSM_PLAN_REPEAT;
}

// ---- steps 3-5 of the update, or the action's progress: the plan of this tick
QR_HD int decide(const qrgpu_fsm_desc &D, Machine &m)
{
    if (m.act != 0) {                                                            // the runner is inside Action::StandUp / SitDown
        const float total = m.act == 1 ? D.stand_up_total : D.sit_down_time;
        return m.act_t < total ? QRGPU_FSM_PLAN_ACTION : (QRGPU_FSM_PLAN_HOLD | QRGPU_FSM_PLAN_ACTION_END);
    }
    command_request(m);
    if (m.req) {                                                                 // RunFSM (:72-94)
        if (m.ctrl == RC_JOY_TROT || m.ctrl == RC_JOY_ADVANCED_TROT || m.ctrl == RC_JOY_WALK || m.ctrl == RC_HARD_CODE) m.fsm_mode = GAIT_TRANSITION;
        else if (m.ctrl == RC_BODY_DOWN) m.fsm_mode = K_STAND_DOWN;
        else if (m.ctrl == RC_BODY_UP) m.fsm_mode = K_STAND_UP;
        else if (m.ctrl == RC_JOY_STAND) m.fsm_mode = LOCOMOTION_STAND;
        else m.fsm_mode = K_PASSIVE;
        m.req = 0;
    }
    if (m.op == OP_NORMAL) {                                                     // :102-114
        int name, run;
        if (m.state == ST_STAND_UP) {                                            // qrFSMStateStandUp::CheckTransition
            m.su_next = ST_STAND_UP;
            if (m.fsm_mode == K_STAND_UP) { if (!m.is_up) m.stand_up = 1; }
            else if (m.fsm_mode == K_STAND_DOWN) { if (m.is_up) m.stand_up = -1; }
            else if (m.fsm_mode == K_LOCOMOTION || m.fsm_mode == LOCOMOTION_STAND || m.fsm_mode == GAIT_TRANSITION) m.su_next = ST_LOCOMOTION;
            else if (m.fsm_mode == K_PASSIVE) m.su_next = ST_PASSIVE;
            name = m.su_next; run = 1;
        } else if (m.state == ST_PASSIVE) {                                      // qrFSMStatePassive::CheckTransition
            m.p_next = ST_PASSIVE;
            if (m.fsm_mode == K_STAND_UP) m.p_next = ST_STAND_UP;
            name = m.p_next; run = 1;
        } else {                                                                 // qrFSMStateLocomotion::CheckTransition
            m.l_iter += 1;
            if (m.fsm_mode == GAIT_TRANSITION) { m.l_dur = D.gait_transition_duration; m.l_iter = 0; }
            else if (m.fsm_mode == LOCOMOTION_STAND) { m.l_dur = D.stand_transition_duration; m.l_iter = 0; }
            else if (m.fsm_mode == K_PASSIVE) { m.l_next = ST_PASSIVE; m.l_dur = 0.f; }
            else if (m.fsm_mode == K_STAND_UP || m.fsm_mode == K_STAND_DOWN) { m.l_next = ST_STAND_UP; m.l_dur = 0.f; }
            name = m.l_next; run = !((double)m.l_dur > 0.1);
        }
        if (name != m.state) { m.op = OP_TRANSITIONING; m.next = name; }
        else if (!run) m.op = OP_TRANSITIONING;
        else {                                                                   // currentState->Run()
            if (m.state == ST_LOCOMOTION) return QRGPU_FSM_PLAN_RUN;
            if (m.state == ST_PASSIVE) return QRGPU_FSM_PLAN_PASSIVE;
            if (m.stand_up != 0) {                                               // the action begins: its first tick
                m.act = m.stand_up; m.act_t = 0.f;
                return QRGPU_FSM_PLAN_ACTION | QRGPU_FSM_PLAN_ACTION_FIRST;
            }
            return QRGPU_FSM_PLAN_HOLD;
        }
    }
    // currentState->Transition() (:117-135)
    if (m.state == ST_STAND_UP) return (m.su_next == ST_LOCOMOTION ? QRGPU_FSM_PLAN_REPEAT : QRGPU_FSM_PLAN_PASSIVE) | QRGPU_FSM_PLAN_DONE;
    if (m.state == ST_PASSIVE) return QRGPU_FSM_PLAN_PASSIVE | QRGPU_FSM_PLAN_DONE;
    if (m.l_next == ST_LOCOMOTION) return self_transition_plan(D, m);
    return (m.l_next == ST_STAND_UP ? QRGPU_FSM_PLAN_REPEAT : QRGPU_FSM_PLAN_PASSIVE) | QRGPU_FSM_PLAN_DONE;
}

// ---- qrgpu_fsm_update_batch, one robot.  msg: the rows of d_joy_msg or null; script rows at stride ns; ticks / done: the robot's words or null.
QR_HD void update(const qrgpu_fsm_desc &D, int reset, size_t S, const float *msg, const float *script, int ns, const int *ticks, const int *done, unsigned bits,
                  float *__restrict__ st, float *__restrict__ joy, int *__restrict__ plan, int *__restrict__ stage_mask)
{
#pragma clang fp contract(off)
    const unsigned dw = done ? ((unsigned)*done & bits) : 0u;
    const bool rst = reset != 0 || dw != 0u;
    Machine m;
    load(D, rst, S, st, m);
    if (rst) {
#pragma unroll
        for (int k = 0; k < QRGPU_MOTOR_CMD_ROWS; ++k) st[(size_t)(S_LAST + k) * S] = 0.f;      // no command sent yet: an empty legCmd
    }
    int btn = 0, have = 0;
    float ax[3] = {0.f, 0.f, 0.f};
    if (msg) {
        float r[QRGPU_JOY_MSG_ROWS];
#pragma unroll
        for (int k = 0; k < QRGPU_JOY_MSG_ROWS; ++k) r[k] = msg[(size_t)k * S];
        if (r[9] != 0.f) m.gait_sw = 1;
        if (r[0] != 0.f) {
            have = 1;
            btn = (r[1] == 1.f ? QRGPU_JOY_BTN_A : 0) | (r[2] == 1.f ? QRGPU_JOY_BTN_B : 0) | (r[3] == 1.f ? QRGPU_JOY_BTN_X : 0) |
                  (r[4] == 1.f ? QRGPU_JOY_BTN_Y : 0) | (r[5] == 1.f ? QRGPU_JOY_BTN_RB : 0);
            ax[0] = r[6]; ax[1] = r[7]; ax[2] = r[8];
        }
    }
    if (script && ticks) {
        const float now = (float)*ticks;
        int hit = 0;
        for (int e = 0; e < ns; ++e) {
            const bool mine = !hit && script[e] == now;
            if (mine) {
                hit = 1;
                const int mask = (int)script[(size_t)ns + e];
                if (mask & QRGPU_JOY_GAIT_SWITCH) m.gait_sw = 1;
                if (!have) {
                    btn = mask; ax[0] = script[(size_t)2 * ns + e]; ax[1] = script[(size_t)3 * ns + e]; ax[2] = script[(size_t)4 * ns + e];
                }
            }
        }
        have |= hit;
    }
    if (have) joy_callback(D, btn, ax, m);
    const int entered = m.entered;
    m.entered = 0;
    const int p = decide(D, m);
    store(S, m, st);
    const bool hard = m.ctrl == RC_HARD_CODE;
#pragma unroll
    for (int k = 0; k < 3; ++k) { joy[(size_t)k * S] = hard ? D.hard_code_v[k] : m.cmd[k]; joy[(size_t)(3 + k) * S] = hard ? D.hard_code_w[k] : m.cmd[3 + k]; }
    joy[6 * S] = D.body_height;
    joy[7 * S] = (float)m.ctrl;
    *plan = p;
    if (stage_mask) *stage_mask = (int)(dw | (entered ? (unsigned)QRGPU_FSM_ENTERED : 0u));
}

// ---- qrgpu_fsm_zero_command_batch, one robot: stateDes.segment(6, 6) = 0 in every copy, where the plan is PHASE1
QR_HD void zero_command(size_t S, int plan, float *__restrict__ des, float *__restrict__ fe, float *__restrict__ fh, float *__restrict__ sv, float *__restrict__ sc)
{
    if (!(plan & QRGPU_FSM_PLAN_PHASE1)) return;
    if (des) {
#pragma unroll
        for (int k = 6; k < 12; ++k) des[(size_t)k * S] = 0.f;
    }
    if (fe) { fe[3 * S] = 0.f; fe[4 * S] = 0.f; fe[5 * S] = 0.f; }
    if (fh) { fh[16 * S] = 0.f; fh[17 * S] = 0.f; fh[18 * S] = 0.f; fh[19 * S] = 0.f; }
    if (sv) { sv[23 * S] = 0.f; sv[24 * S] = 0.f; sv[25 * S] = 0.f; sv[26 * S] = 0.f; }
    if (sc) {
#pragma unroll
        for (int k = 1; k < 7; ++k) sc[(size_t)k * S] = 0.f;
    }
}

// OnEnter of the state just entered (qr_fsm_state_passive.cpp:40-44, qr_fsm_state_standup.cpp:42-54, qr_fsm_state_locomotion.cpp:78-126)
QR_HD void on_enter(Machine &m)
{
    if (m.state == ST_PASSIVE) { m.p_next = ST_PASSIVE; m.p_done = 0; }
    else if (m.state == ST_STAND_UP) { m.su_next = ST_STAND_UP; m.su_done = 0; m.stand_up = 1; m.fsm_mode = K_STAND_UP; }
    else {
        m.l_next = ST_LOCOMOTION; m.l_done = 0;
        if (m.ctrl != RC_HARD_CODE) {
            if (m.ctrl == RC_JOY_TROT) { m.mode = MODE_VELOCITY; m.gait = QRGPU_FSM_GAIT_TROT; }
            else if (m.ctrl == RC_JOY_ADVANCED_TROT) { m.mode = MODE_ADVANCED_TROT; m.gait = QRGPU_FSM_GAIT_ADVANCED_TROT; }
            else if (m.ctrl == RC_JOY_WALK) { m.mode = MODE_WALK; m.gait = QRGPU_FSM_GAIT_WALK; }
            else m.gait = QRGPU_FSM_GAIT_STAND;
            m.entered = 1;                                                       // quadruped->Reset(), locomotionController->Reset(), stateEstimators->Reset()
        }
    }
}

// ---- qrgpu_fsm_command_batch, one robot.  ein: est_in (contacts 13-16, motor angles 17-28); loco may be cmd itself: every load is made before the first store.
QR_HD void command(const qrgpu_fsm_desc &D, size_t S, int plan, const float *ein, const float *loco, float *__restrict__ st, float *cmd, float *__restrict__ out)
{
#pragma clang fp contract(off)
    Machine m;
    load(D, false, S, st, m);
    float q[12], c[QRGPU_MOTOR_CMD_ROWS], last[QRGPU_MOTOR_CMD_ROWS];
    int N = 0;
#pragma unroll
    for (int l = 0; l < 4; ++l) N += ein[(size_t)(13 + l) * S] != 0.f ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) q[k] = ein[(size_t)(17 + k) * S];
#pragma unroll
    for (int k = 0; k < QRGPU_MOTOR_CMD_ROWS; ++k) { c[k] = loco[(size_t)k * S]; last[k] = st[(size_t)(S_LAST + k) * S]; }
    const int T = D.transition_ticks;
    const int kind = plan & PLAN_KINDS;
    const bool self = m.state == ST_LOCOMOTION && m.op == OP_TRANSITIONING && m.l_next == ST_LOCOMOTION;
    float p[12];
    bool pd = false;                                                             // the command is {p, Kp, 0, Kd, 0}
    if (kind == QRGPU_FSM_PLAN_RUN || kind == QRGPU_FSM_PLAN_PHASE1) {
        // the locomotion column as it is
    } else if (kind == QRGPU_FSM_PLAN_PHASE2) {                                  // :303-307
        const float r0 = (float)(m.l_iter - T) / (float)T;
        const float ratio = 0.45f < r0 ? r0 : 0.45f;                             // std::max(0.45f, r0)
#pragma unroll
        for (int k = 0; k < 12; ++k) p[k] = D.stand_up_angles[k] * ratio + (1.f - ratio) * q[k];
        pd = true;
    } else if (kind == QRGPU_FSM_PLAN_ACTION) {
        if (plan & QRGPU_FSM_PLAN_ACTION_FIRST) {
#pragma unroll
            for (int k = 0; k < 12; ++k) m.qb[k] = q[k];
        }
        if (m.act == 1) {                                                        // Action::StandUp (:45-70)
            const float blend = m.act_t / D.stand_up_time;
#pragma unroll
            for (int k = 0; k < 12; ++k) p[k] = blend < 1.0f ? blend * D.stand_up_angles[k] + (1.f - blend) * m.qb[k] : D.stand_up_angles[k];
        } else {                                                                 // Action::SitDown (:88-93)
            const float blend = m.act_t / D.sit_down_time;
#pragma unroll
            for (int k = 0; k < 12; ++k) p[k] = blend * D.sit_down_angles[k] + (1.f - blend) * m.qb[k];
        }
        m.act_t = m.act_t + D.time_step;
        pd = true;
    } else if (kind == QRGPU_FSM_PLAN_HOLD) {                                    // qr_fsm_state_standup.cpp:61-81
        if (plan & QRGPU_FSM_PLAN_ACTION_END) { m.is_up = m.act == 1 ? 1 : 0; m.act = 0; }
        m.stand_up = 0;
#pragma unroll
        for (int k = 0; k < 12; ++k) p[k] = m.is_up ? D.stand_up_angles[k] : D.sit_down_angles[k];
        pd = true;
    } else if (kind == QRGPU_FSM_PLAN_REPEAT) {
#pragma unroll
        for (int k = 0; k < QRGPU_MOTOR_CMD_ROWS; ++k) c[k] = last[k];
    } else {                                                                     // PASSIVE; an empty legCommand
#pragma unroll
        for (int k = 0; k < QRGPU_MOTOR_CMD_ROWS; ++k) c[k] = 0.f;
    }
    if (pd) {
#pragma unroll
        for (int k = 0; k < 12; ++k) { c[k] = p[k]; c[12 + k] = D.kp[k]; c[24 + k] = 0.f; c[36 + k] = D.kd[k]; c[48 + k] = 0.f; }
    }
    if (self) {                                                                  // SwitchMode / StandLoop, then Transition's iter++ (:239)
        if (plan & QRGPU_FSM_PLAN_DONE) { m.fsm_mode = K_LOCOMOTION; m.l_iter = 0; m.l_done = 1; m.l_dur = 0.f; }
        else if (kind == QRGPU_FSM_PLAN_PHASE1 && N == 4) m.l_iter = T;
        m.l_iter += 1;
    } else if (plan & QRGPU_FSM_PLAN_DONE) {                                     // the other Transition()s
        if (m.state == ST_STAND_UP) m.su_done = 1;
        else if (m.state == ST_PASSIVE) m.p_done = 1;
        else { m.l_done = 1; if (m.l_next == ST_PASSIVE) m.l_checks = 0; }       // TurnOffAllSafetyChecks (:250)
    }
    if (m.state == ST_LOCOMOTION && m.l_checks) {                                // SafetyPostCheck: CheckForceFeedForward
        const float lim = D.tau_clip;
#pragma unroll
        for (int k = 48; k < 60; ++k) c[k] = c[k] > lim ? lim : (c[k] < -lim ? -lim : c[k]);
    }
    if (plan & QRGPU_FSM_PLAN_DONE) {                                            // :126-135
        if (m.state == ST_LOCOMOTION) m.l_iter = 0;                              // OnExit
        m.state = m.next;
        on_enter(m);
        m.op = OP_NORMAL;
    }
    store(S, m, st);
#pragma unroll
    for (int k = 0; k < QRGPU_MOTOR_CMD_ROWS; ++k) { st[(size_t)(S_LAST + k) * S] = c[k]; cmd[(size_t)k * S] = c[k]; }
    if (out) {
        const int on = m.state == ST_LOCOMOTION && m.l_checks;
        out[0] = (float)m.state; out[S] = (float)m.op; out[2 * S] = (float)m.fsm_mode; out[3 * S] = (float)m.ctrl; out[4 * S] = (float)m.l_iter;
        out[5 * S] = (float)on; out[6 * S] = 0.f; out[7 * S] = (float)on;
        out[8 * S] = (float)m.gait; out[9 * S] = (float)m.mode; out[10 * S] = (float)m.act;
    }
}

}  // namespace fsm
}  // namespace qrgpu
