// K11 family: one step of all worlds of a multi-agent particle scenario as ONE launch (row f1 of the scope table: the
// device-resident rollout loop).  The worlds (reference onpolicy/envs/mpe/core.py:120-190 physics, environment.py:100-255
// step / action decoding, scenarios/*.py reward / observation) are a few dozen float64 operations per agent pair.
// Written as array operations on device tensors a step is ~60 small launches (measured for simple_spread: 140 ms per
// step at 4096 worlds, ten times slower than the numpy env on the host); here a thread owns a world and keeps its
// entities in registers.  State is float64 like the reference's numpy physics and is advanced in place, observations and
// rewards leave as float32.  Restarted worlds take their state from `fresh_*`, draws the caller makes every step
// (branch-free: drawn for all worlds, used where a world restarts), so the trajectories are those of the tensor
// implementation (envs/mpe/*.py::_step_ops) for the same generator.
//
// The particle physics every scenario shares is written once (World and the helpers below); a scenario's kernel adds its
// own forces, extra state, reward and observation.  A world's entities are plain arrays px / py / vx / vy [agents] and
// lx / ly [landmarks] that the helpers take by reference (separate arrays: one aggregate of all six does not come apart
// into registers at 16 entities); they are templated on the array bound so that a scenario with fixed counts keeps them
// at compile time and one with runtime counts stays fully unrolled.
#include <hip/hip_runtime.h>

#include "../../include/mappo_hip.h"
#include "mappo_internal.h"

namespace {

constexpr int kMax = MAPPO_ENV_MAX_ENTITIES;
constexpr double kDt = 0.1, kDamping = 0.25, kSens = 5.0, kForce = 1e2, kMargin = 1e-3, kSize = 0.15;

// what the step of any particle world takes (A agents, L landmarks)
struct World {
    double* pos;                // [N, A, 2]
    double* vel;                // [N, A, 2]
    double* land;               // [N, L, 2]
    long long* t;               // [N]
    const double* fresh_pos;    // [N, A, 2] uniform(-1, 1)
    const double* fresh_land;   // [N, L, 2] uniform(-1, 1)
    float* obs;                 // [N, A, Do] ([N, sum Do] where the agents' observations differ in width)
    float* rew;                 // [N, A, 1]
    unsigned char* done;        // [N, A] (bool)
    double* per_agent;          // [N, A]
    long long n;
    int world_length, auto_reset;
};

template <int M>
__device__ __forceinline__ void load_xy(const double* src, long long w, int count, double (&x)[M], double (&y)[M]) {
#pragma unroll
    for (int i = 0; i < M; ++i) {
        if (i >= count) continue;
        x[i] = src[(w * count + i) * 2];
        y[i] = src[(w * count + i) * 2 + 1];
    }
}

template <int M>
__device__ __forceinline__ void store_xy(double* dst, long long w, int count, const double (&x)[M],
                                         const double (&y)[M]) {
#pragma unroll
    for (int i = 0; i < M; ++i) {
        if (i >= count) continue;
        dst[(w * count + i) * 2] = x[i];
        dst[(w * count + i) * 2 + 1] = y[i];
    }
}

template <int MA, int ML>
__device__ __forceinline__ void load_world(const World& s, long long w, int A, int L, double (&px)[MA],
                                           double (&py)[MA], double (&vx)[MA], double (&vy)[MA], double (&lx)[ML],
                                           double (&ly)[ML]) {
    load_xy(s.pos, w, A, px, py);
    load_xy(s.vel, w, A, vx, vy);
    load_xy(s.land, w, L, lx, ly);
}

// movement index -> force (environment.py: u[0] += a[1] - a[2], u[1] += a[3] - a[4], x sensitivity; an agent with an
// acceleration of its own is scaled by that instead)
__device__ __forceinline__ void action_force(long long mv, double& fx, double& fy, double scale = kSens) {
    fx = (mv == 1 ? 1.0 : mv == 2 ? -1.0 : 0.0) * scale;
    fy = (mv == 3 ? 1.0 : mv == 4 ? -1.0 : 0.0) * scale;
}

// a property that the adversaries (agents before `n_adv`) and the good agents of a scenario hold different values of.
// A scenario whose agents are all alike passes n_adv = 0 as a literal, and the choice folds away
struct ByKind {
    int n_adv;
    double adversary, good;
    __device__ __forceinline__ double of(int i) const { return i < n_adv ? adversary : good; }
};

// the force of one soft contact on the entity at distance (dx, dy) from the other, which collide below `dist_min`, the
// sum of their radii (core.py:296-314 get_collision_force: softmax penetration, force along the line between the two)
__device__ __forceinline__ void contact_force(double dx, double dy, double dist_min, double& sx, double& sy) {
    const double dist = sqrt(dx * dx + dy * dy);
    const double x = -(dist - dist_min) / kMargin;
    const double pen = (fmax(x, 0.0) + log1p(exp(-fabs(x)))) * kMargin;     // logaddexp(0, x) * margin
    double gx = kForce * dx / dist * pen, gy = kForce * dy / dist * pen;
    if (!isfinite(gx)) gx = 0.0;                                             // coincident centres: no force
    if (!isfinite(gy)) gy = 0.0;
    sx += gx;
    sy += gy;
}

// soft contacts between agents of radius `size`, added to the force on each agent
template <int MA>
__device__ __forceinline__ void add_contact_forces(int A, const ByKind& size, const double (&px)[MA],
                                                   const double (&py)[MA], double (&fx)[MA], double (&fy)[MA]) {
#pragma unroll
    for (int i = 0; i < MA; ++i) {
        if (i >= A) continue;
        double sx = 0.0, sy = 0.0;
#pragma unroll
        for (int j = 0; j < MA; ++j) {
            if (j >= A || j == i) continue;
            contact_force(px[i] - px[j], py[i] - py[j], size.of(i) + size.of(j), sx, sy);
        }
        fx[i] += sx;
        fy[i] += sy;
    }
}

// soft contacts of the agents with landmarks of radius `land_size` that collide and never move (core.py:318-320): the
// agent alone takes the force, away from the landmark
template <int MA, int ML>
__device__ __forceinline__ void add_landmark_contact_forces(int A, int L, const ByKind& size, double land_size,
                                                            const double (&px)[MA], const double (&py)[MA],
                                                            const double (&lx)[ML], const double (&ly)[ML],
                                                            double (&fx)[MA], double (&fy)[MA]) {
#pragma unroll
    for (int i = 0; i < MA; ++i) {
        if (i >= A) continue;
        double sx = 0.0, sy = 0.0;
#pragma unroll
        for (int l = 0; l < ML; ++l) {
            if (l >= L) continue;
            contact_force(px[i] - lx[l], py[i] - ly[l], size.of(i) + land_size, sx, sy);
        }
        fx[i] += sx;
        fy[i] += sy;
    }
}

// core.py:265-278: damping, then force * dt (every mass is 1), then -- kClamp, for scenarios whose agents have one -- the
// top speed `max_speed`, then the position.  Agents before `first` are not movable (core.py:267) and keep their position
// and velocity
template <bool kClamp = false, int MA>
__device__ __forceinline__ void integrate(int A, double (&px)[MA], double (&py)[MA], double (&vx)[MA], double (&vy)[MA],
                                          const double (&fx)[MA], const double (&fy)[MA], int first = 0,
                                          const ByKind& max_speed = ByKind{0, 0.0, 0.0}) {
#pragma unroll
    for (int i = 0; i < MA; ++i) {
        if (i < first || i >= A) continue;
        vx[i] = vx[i] * (1 - kDamping) + fx[i] * kDt;
        vy[i] = vy[i] * (1 - kDamping) + fy[i] * kDt;
        if (kClamp) {
            const double speed = sqrt(vx[i] * vx[i] + vy[i] * vy[i]), top = max_speed.of(i);
            if (speed > top) {
                vx[i] = vx[i] / speed * top;
                vy[i] = vy[i] / speed * top;
            }
        }
        px[i] = px[i] + vx[i] * kDt;
        py[i] = py[i] + vy[i] * kDt;
    }
}

// individual rewards, the reward each agent is paid and the done flag of a world whose clock now shows t; -> the world
// restarts.  A collaborative world (environment.py:141-143 shared_reward) pays every agent `total`, any other its own
template <int MA>
__device__ __forceinline__ bool write_outcome(const World& s, long long w, int A, long long t, const double (&pa)[MA],
                                              double total, bool shared = true) {
    const bool done = t >= s.world_length;
#pragma unroll
    for (int i = 0; i < MA; ++i) {
        if (i >= A) continue;
        s.per_agent[w * A + i] = pa[i];
        s.rew[w * A + i] = (float)(shared ? total : pa[i]);
        s.done[w * A + i] = done ? 1 : 0;
    }
    return done && s.auto_reset;
}

// a restarting world: agents at fresh_pos and at rest, landmarks at land_scale * fresh_land
template <int MA, int ML>
__device__ __forceinline__ void restart_from_fresh(const World& s, long long w, int A, int L, double land_scale,
                                                   double (&px)[MA], double (&py)[MA], double (&vx)[MA],
                                                   double (&vy)[MA], double (&lx)[ML], double (&ly)[ML]) {
    load_xy(s.fresh_pos, w, A, px, py);
    load_xy(s.fresh_land, w, L, lx, ly);
#pragma unroll
    for (int i = 0; i < MA; ++i) {
        if (i < A) vx[i] = vy[i] = 0.0;
    }
#pragma unroll
    for (int l = 0; l < ML; ++l) {
        if (l >= L) continue;
        lx[l] = land_scale * lx[l];
        ly[l] = land_scale * ly[l];
    }
}

// landmarks move only when a world restarts
template <int MA, int ML>
__device__ __forceinline__ void store_world(const World& s, long long w, int A, int L, long long t, bool restart,
                                            const double (&px)[MA], const double (&py)[MA],
                                            const double (&vx)[MA], const double (&vy)[MA],
                                            const double (&lx)[ML], const double (&ly)[ML]) {
    s.t[w] = t;
    store_xy(s.pos, w, A, px, py);
    store_xy(s.vel, w, A, vx, vy);
    if (restart) store_xy(s.land, w, L, lx, ly);
}

// ------------------------------------------------------------------------------------------------------------------
// simple_spread (cooperative navigation; scenarios/simple_spread.py:60-103): A agents, L landmarks, soft contacts
struct Args {
    World s;
    const long long* act;   // [N, A] action indices 0..4
    int A, L;               // Do = 4 + 2 L + 4 (A - 1)
};

__global__ void __launch_bounds__(64) spread_step_kernel(Args a) {
    const long long w = (long long)blockIdx.x * 64 + threadIdx.x;
    const World& s = a.s;
    if (w >= s.n) return;
    const int A = a.A, L = a.L;
    double px[kMax], py[kMax], vx[kMax], vy[kMax], lx[kMax], ly[kMax];
    load_world(s, w, A, L, px, py, vx, vy, lx, ly);
    // ---- forces: action + soft contacts
    double fx[kMax], fy[kMax];
#pragma unroll
    for (int i = 0; i < kMax; ++i) {
        if (i < A) action_force(a.act[w * A + i], fx[i], fy[i]);
    }
    add_contact_forces(A, ByKind{0, kSize, kSize}, px, py, fx, fy);
    integrate(A, px, py, vx, vy, fx, fy);
    long long t = s.t[w] + 1;
    // ---- reward (simple_spread.py:60-84): -sum over landmarks of the closest agent's distance, -1 per contact
    double cover = 0.0;
#pragma unroll
    for (int l = 0; l < kMax; ++l) {
        if (l >= L) continue;
        double best = 1e300;
#pragma unroll
        for (int i = 0; i < kMax; ++i) {
            if (i >= A) continue;
            const double dx = px[i] - lx[l], dy = py[i] - ly[l];
            best = fmin(best, sqrt(dx * dx + dy * dy));
        }
        cover -= best;
    }
    double total = 0.0;
    double pa[kMax];
#pragma unroll
    for (int i = 0; i < kMax; ++i) {
        if (i >= A) continue;
        int hits = 0;
#pragma unroll
        for (int j = 0; j < kMax; ++j) {
            if (j >= A) continue;
            const double dx = px[i] - px[j], dy = py[i] - py[j];
            hits += sqrt(dx * dx + dy * dy) < 2 * kSize;        // the agent itself included, as in the reference
        }
        pa[i] = cover - hits;
        total += pa[i];
    }
    const bool restart = write_outcome(s, w, A, t, pa, total);
    if (restart) {
        t = 0;
        restart_from_fresh(s, w, A, L, 1.0, px, py, vx, vy, lx, ly);
    }
    store_world(s, w, A, L, t, restart, px, py, vx, vy, lx, ly);
    // ---- observation of the (possibly restarted) world: vel, pos, landmarks and other agents relative to the agent,
    // (A - 1) * 2 zero communication channels (simple_spread.py:86-103)
    const int Do = 4 + 2 * L + 4 * (A - 1);
#pragma unroll
    for (int i = 0; i < kMax; ++i) {
        if (i >= A) continue;
        float* o = s.obs + (w * A + i) * Do;
        int k = 0;
        o[k++] = (float)vx[i];
        o[k++] = (float)vy[i];
        o[k++] = (float)px[i];
        o[k++] = (float)py[i];
#pragma unroll
        for (int l = 0; l < kMax; ++l) {
            if (l >= L) continue;
            o[k++] = (float)(lx[l] - px[i]);
            o[k++] = (float)(ly[l] - py[i]);
        }
#pragma unroll
        for (int j = 0; j < kMax; ++j) {
            if (j >= A || j == i) continue;
            o[k++] = (float)(px[j] - px[i]);
            o[k++] = (float)(py[j] - py[i]);
        }
        for (int z = 0; z < 2 * (A - 1); ++z) o[k++] = 0.f;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// simple_reference (referential communication; scenarios/simple_reference.py, core.py:207-288 communication state):
// two agents, three landmarks, no contacts.  Each agent carries the goal landmark the OTHER agent has to reach and the
// index of its last communication symbol (-1: silent), both advanced in place like the physics.
constexpr int kRefAgents = 2, kRefLandmarks = 3, kRefSymbols = 10;
constexpr int kRefObs = 2 + 2 * kRefLandmarks + 3 + kRefSymbols;     // 21
constexpr double kRefLandmarkScale = 0.8;

struct RefArgs {
    World s;
    long long* goal;                // [N, 2] goal landmark of each agent, 0..2
    long long* comm;                // [N, 2] last symbol of each agent, -1 = silent
    const long long* act;           // [N, 2, 2] (movement 0..4, symbol 0..9)
    const long long* fresh_goal;    // [N, 2] 0..2
};

__global__ void __launch_bounds__(64) reference_step_kernel(RefArgs a) {
    const long long w = (long long)blockIdx.x * 64 + threadIdx.x;
    const World& s = a.s;
    if (w >= s.n) return;
    constexpr int A = kRefAgents, L = kRefLandmarks;
    double px[A], py[A], vx[A], vy[A], lx[L], ly[L];
    load_world(s, w, A, L, px, py, vx, vy, lx, ly);
    long long goal[A], comm[A];
    // ---- action force and integration; the symbol becomes the communication state
    double fx[A], fy[A];
#pragma unroll
    for (int i = 0; i < A; ++i) {
        goal[i] = a.goal[w * A + i];
        action_force(a.act[(w * A + i) * 2], fx[i], fy[i]);
        comm[i] = a.act[(w * A + i) * 2 + 1];
    }
    integrate(A, px, py, vx, vy, fx, fy);
    long long t = s.t[w] + 1;
    // ---- reward (simple_reference.py: -|goal_a - goal_b|^2, goal_a = the other agent), shared as r_0 + r_1
    double pa[A];
#pragma unroll
    for (int i = 0; i < A; ++i) {
        const int o = A - 1 - i;
        const long long g = goal[i];
        const double gx = g == 0 ? lx[0] : g == 1 ? lx[1] : lx[2];
        const double gy = g == 0 ? ly[0] : g == 1 ? ly[1] : ly[2];
        const double dx = px[o] - gx, dy = py[o] - gy;
        pa[i] = -(dx * dx + dy * dy);
    }
    const bool restart = write_outcome(s, w, A, t, pa, pa[0] + pa[1]);
    if (restart) {
        t = 0;
        restart_from_fresh(s, w, A, L, kRefLandmarkScale, px, py, vx, vy, lx, ly);
    }
    store_world(s, w, A, L, t, restart, px, py, vx, vy, lx, ly);
#pragma unroll
    for (int i = 0; i < A; ++i) {
        if (restart) {
            goal[i] = a.fresh_goal[w * A + i];
            comm[i] = -1;
            a.goal[w * A + i] = goal[i];
        }
        a.comm[w * A + i] = comm[i];
    }
    // ---- observation of the (possibly restarted) world (simple_reference.py observation): own velocity, landmarks
    // relative to the agent, the colour of the agent's goal landmark, the other agent's communication state (one-hot)
#pragma unroll
    for (int i = 0; i < A; ++i) {
        float* o = s.obs + (w * A + i) * kRefObs;
        int k = 0;
        o[k++] = (float)vx[i];
        o[k++] = (float)vy[i];
#pragma unroll
        for (int l = 0; l < L; ++l) {
            o[k++] = (float)(lx[l] - px[i]);
            o[k++] = (float)(ly[l] - py[i]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) o[k++] = goal[i] == c ? 0.75f : 0.25f;     // palette: 0.75 on the landmark's own channel
        const long long heard = comm[A - 1 - i];
#pragma unroll
        for (int sym = 0; sym < kRefSymbols; ++sym) o[k++] = heard == sym ? 1.f : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// simple_speaker_listener (scenarios/simple_speaker_listener.py): agent 0, the speaker, does not move and sees the colour
// of the goal landmark; agent 1, the listener, is silent and has to reach it.  One goal and one communication symbol per
// world (the speaker's; -1: silent), advanced in place like simple_reference's.  The observation leaves as ONE row per
// world, speaker's columns first: what the centralised critic reads, and column views of it are the agents' own.
constexpr int kSpkAgents = 2, kSpkLandmarks = 3, kSpkSymbols = 3, kSpeaker = 0, kListener = 1;
constexpr int kSpkObs = 3 + (2 + 2 * kSpkLandmarks + kSpkSymbols);     // 3 + 11 = 14

struct SpeakerArgs {
    World s;                        // s.obs: [N, 14]
    long long* goal;                // [N] goal landmark, 0..2
    long long* comm;                // [N] the speaker's last symbol, -1 = silent
    const long long* act;           // [N, 2] (the speaker's symbol 0..2, the listener's movement 0..4)
    const long long* fresh_goal;    // [N] 0..2
};

__global__ void __launch_bounds__(64) speaker_listener_step_kernel(SpeakerArgs a) {
    const long long w = (long long)blockIdx.x * 64 + threadIdx.x;
    const World& s = a.s;
    if (w >= s.n) return;
    constexpr int A = kSpkAgents, L = kSpkLandmarks;
    double px[A], py[A], vx[A], vy[A], lx[L], ly[L];
    load_world(s, w, A, L, px, py, vx, vy, lx, ly);
    long long goal = a.goal[w];
    // ---- the symbol becomes the communication state; only the listener takes a force and is integrated
    long long comm = a.act[w * A + kSpeaker];
    double fx[A] = {0.0, 0.0}, fy[A] = {0.0, 0.0};
    action_force(a.act[w * A + kListener], fx[kListener], fy[kListener]);
    integrate(A, px, py, vx, vy, fx, fy, kListener);
    long long t = s.t[w] + 1;
    // ---- reward (simple_speaker_listener.py:69-73): -|listener - goal landmark|^2 for both agents, shared as their sum
    const double gx = goal == 0 ? lx[0] : goal == 1 ? lx[1] : lx[2];
    const double gy = goal == 0 ? ly[0] : goal == 1 ? ly[1] : ly[2];
    const double dx = px[kListener] - gx, dy = py[kListener] - gy;
    double pa[A];
    pa[0] = pa[1] = -(dx * dx + dy * dy);
    const bool restart = write_outcome(s, w, A, t, pa, pa[0] + pa[1]);
    if (restart) {
        t = 0;
        restart_from_fresh(s, w, A, L, 1.0, px, py, vx, vy, lx, ly);
        goal = a.fresh_goal[w];
        comm = -1;
        a.goal[w] = goal;
    }
    store_world(s, w, A, L, t, restart, px, py, vx, vy, lx, ly);
    a.comm[w] = comm;
    // ---- observation of the (possibly restarted) world (simple_speaker_listener.py:75-98).  Speaker: the goal landmark's
    // colour (palette: 0.65 on the landmark's own channel); listener: own velocity, landmarks relative to it, the
    // speaker's communication state (one-hot)
    float* o = s.obs + w * kSpkObs;
    int k = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[k++] = goal == c ? 0.65f : 0.15f;
    o[k++] = (float)vx[kListener];
    o[k++] = (float)vy[kListener];
#pragma unroll
    for (int l = 0; l < L; ++l) {
        o[k++] = (float)(lx[l] - px[kListener]);
        o[k++] = (float)(ly[l] - py[kListener]);
    }
#pragma unroll
    for (int sym = 0; sym < kSpkSymbols; ++sym) o[k++] = comm == sym ? 1.f : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------
// simple_push (keep-away; scenarios/simple_push.py): agent 0, the adversary, has to keep the good agents 1..A-1 away from
// the goal landmark all of them share; every agent moves, is silent and collides (radius 0.05).  Not collaborative: each
// agent is paid its own reward.  One goal per world, advanced in place like simple_speaker_listener's; the observation
// leaves as ONE row per world, adversary's columns first, then the good agents' in agent order.
constexpr int kPushLandmarks = 2;           // the landmark palette has a channel for two (simple_push.py:43-45)
constexpr double kPushSize = 0.05, kPushLandmarkScale = 0.8;

struct PushArgs {
    World s;                        // s.obs: [N, (2 + 2 L + 2 (A - 1)) + (A - 1) (7 + 5 L + 2 (A - 1))]
    long long* goal;                // [N] goal landmark, 0..L-1
    const long long* act;           // [N, A] action indices 0..4
    const long long* fresh_goal;    // [N] 0..L-1
    int A, L;
};

__global__ void __launch_bounds__(64) push_step_kernel(PushArgs a) {
    const long long w = (long long)blockIdx.x * 64 + threadIdx.x;
    const World& s = a.s;
    if (w >= s.n) return;
    const int A = a.A, L = a.L;
    constexpr int ML = kPushLandmarks;
    double px[kMax], py[kMax], vx[kMax], vy[kMax], lx[ML] = {0.0, 0.0}, ly[ML] = {0.0, 0.0};
    load_world(s, w, A, L, px, py, vx, vy, lx, ly);
    long long goal = a.goal[w];
    // ---- forces: action + soft contacts
    double fx[kMax], fy[kMax];
#pragma unroll
    for (int i = 0; i < kMax; ++i) {
        if (i < A) action_force(a.act[w * A + i], fx[i], fy[i]);
    }
    add_contact_forces(A, ByKind{0, kPushSize, kPushSize}, px, py, fx, fy);
    integrate(A, px, py, vx, vy, fx, fy);
    long long t = s.t[w] + 1;
    // ---- reward (simple_push.py:66-82): a good agent -|pos - goal|, the adversary the closest good agent's distance to
    // the goal minus its own
    {
        const double gx = goal == 0 ? lx[0] : lx[1], gy = goal == 0 ? ly[0] : ly[1];
        double pa[kMax];
        double own = 0.0, nearest = 1e300;
#pragma unroll
        for (int i = 0; i < kMax; ++i) {
            if (i >= A) continue;
            const double dx = px[i] - gx, dy = py[i] - gy;
            const double d = sqrt(dx * dx + dy * dy);
            pa[i] = -d;
            if (i == 0) own = d; else nearest = fmin(nearest, d);
        }
        pa[0] = nearest - own;
        const bool restart = write_outcome(s, w, A, t, pa, 0.0, false);
        if (restart) {
            t = 0;
            restart_from_fresh(s, w, A, L, kPushLandmarkScale, px, py, vx, vy, lx, ly);
            goal = a.fresh_goal[w];
            a.goal[w] = goal;
        }
        store_world(s, w, A, L, t, restart, px, py, vx, vy, lx, ly);
    }
    // ---- observation of the (possibly restarted) world (simple_push.py:84-104).  Adversary: own velocity, landmarks and
    // other agents relative to it.  Good agent: own velocity, the goal relative to it, own colour (0.75 on the goal's
    // channel), landmarks relative to it, the landmarks' colours (0.9 on a landmark's own channel), other agents
    const double gx = goal == 0 ? lx[0] : lx[1], gy = goal == 0 ? ly[0] : ly[1];
    const int Da = 2 + 2 * L + 2 * (A - 1), Dg = 7 + 5 * L + 2 * (A - 1);
    float* row = s.obs + w * (Da + (long long)(A - 1) * Dg);
#pragma unroll
    for (int i = 0; i < kMax; ++i) {
        if (i >= A) continue;
        float* o = i == 0 ? row : row + Da + (i - 1) * Dg;
        int k = 0;
        o[k++] = (float)vx[i];
        o[k++] = (float)vy[i];
        if (i > 0) {
            o[k++] = (float)(gx - px[i]);
            o[k++] = (float)(gy - py[i]);
            o[k++] = 0.25f;
            o[k++] = goal == 0 ? 0.75f : 0.25f;
            o[k++] = goal == 1 ? 0.75f : 0.25f;
        }
#pragma unroll
        for (int l = 0; l < ML; ++l) {
            if (l >= L) continue;
            o[k++] = (float)(lx[l] - px[i]);
            o[k++] = (float)(ly[l] - py[i]);
        }
        if (i > 0) {
#pragma unroll
            for (int l = 0; l < ML; ++l) {
                if (l >= L) continue;
                o[k++] = 0.1f;
                o[k++] = l == 0 ? 0.9f : 0.1f;
                o[k++] = l == 1 ? 0.9f : 0.1f;
            }
        }
#pragma unroll
        for (int j = 0; j < kMax; ++j) {
            if (j >= A || j == i) continue;
            o[k++] = (float)(px[j] - px[i]);
            o[k++] = (float)(py[j] - py[i]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// simple_tag (predator-prey; scenarios/simple_tag.py): agents 0..Nadv-1, the adversaries, chase the good agents Nadv..A-1
// among landmarks that collide and never move.  An adversary is large and slow, a good agent small and fast; every agent
// moves, is silent, collides and has a top speed.  Not collaborative: each agent is paid its own reward.  No state besides
// the particle state; the observation leaves as ONE row per world, the agents' columns in agent order.
constexpr int kTagLandmarks = MAPPO_TAG_MAX_LANDMARKS;
constexpr double kTagLandmarkScale = 0.8, kTagLandmarkSize = 0.2, kTagCatch = 10.0;
// (adversary, good agent)
constexpr double kTagSize[2] = {0.075, 0.05}, kTagAccel[2] = {3.0, 4.0}, kTagMaxSpeed[2] = {1.0, 1.3};

struct TagArgs {
    World s;                        // s.obs: [N, Nadv (4 + 2 L + 2 (A - 1) + 2 G) + G (4 + 2 L + 2 (A - 1) + 2 (G - 1))], G = A - Nadv
    const long long* act;           // [N, A] action indices 0..4
    int A, n_adv, L;
};

// the penalty for leaving the screen along one axis (simple_tag.py:100-105), x = |coordinate|
__device__ __forceinline__ double tag_bound(double x) {
    return x < 0.9 ? 0.0 : x < 1.0 ? (x - 0.9) * 10 : fmin(exp(2 * x - 2), 10.0);
}

__global__ void __launch_bounds__(64) tag_step_kernel(TagArgs a) {
    const long long w = (long long)blockIdx.x * 64 + threadIdx.x;
    const World& s = a.s;
    if (w >= s.n) return;
    const int A = a.A, L = a.L, n_adv = a.n_adv;
    constexpr int ML = kTagLandmarks;
    double px[kMax], py[kMax], vx[kMax], vy[kMax], lx[ML], ly[ML];
    load_world(s, w, A, L, px, py, vx, vy, lx, ly);
    const ByKind size{n_adv, kTagSize[0], kTagSize[1]};
    // ---- forces: action (the acceleration acts twice: as the action's sensitivity, environment.py:233-236, and as the
    // force's factor, core.py:236-237) + soft contacts with agents and landmarks
    {
        const ByKind scale{n_adv, kTagAccel[0] * kTagAccel[0], kTagAccel[1] * kTagAccel[1]};
        double fx[kMax], fy[kMax];
#pragma unroll
        for (int i = 0; i < kMax; ++i) {
            if (i < A) action_force(a.act[w * A + i], fx[i], fy[i], scale.of(i));
        }
        add_contact_forces(A, size, px, py, fx, fy);
        add_landmark_contact_forces(A, L, size, kTagLandmarkSize, px, py, lx, ly, fx, fy);
        integrate<true>(A, px, py, vx, vy, fx, fy, 0, ByKind{n_adv, kTagMaxSpeed[0], kTagMaxSpeed[1]});
    }
    long long t = s.t[w] + 1;
    // ---- reward (simple_tag.py:86-126): a good agent -10 per adversary that touches it and the penalty for leaving the
    // screen, every adversary +10 per (good agent, adversary) pair in touch, whoever the adversary
    {
        double pa[kMax];
        int hits = 0;
#pragma unroll
        for (int g = 0; g < kMax; ++g) {
            if (g < n_adv || g >= A) continue;
            int mine = 0;
#pragma unroll
            for (int j = 0; j < kMax; ++j) {
                if (j >= n_adv || j >= A) continue;
                const double dx = px[g] - px[j], dy = py[g] - py[j];
                mine += sqrt(dx * dx + dy * dy) < kTagSize[1] + kTagSize[0];
            }
            hits += mine;
            pa[g] = -kTagCatch * mine - (tag_bound(fabs(px[g])) + tag_bound(fabs(py[g])));
        }
#pragma unroll
        for (int i = 0; i < kMax; ++i) {
            if (i < n_adv) pa[i] = kTagCatch * hits;
        }
        const bool restart = write_outcome(s, w, A, t, pa, 0.0, false);
        if (restart) {
            t = 0;
            restart_from_fresh(s, w, A, L, kTagLandmarkScale, px, py, vx, vy, lx, ly);
        }
        store_world(s, w, A, L, t, restart, px, py, vx, vy, lx, ly);
    }
    // ---- observation of the (possibly restarted) world (simple_tag.py:128-144): own velocity, own position, landmarks
    // and other agents relative to the agent, the velocities of the other good agents
    const int G = A - n_adv;
    const int Da = 4 + 2 * L + 2 * (A - 1) + 2 * G, Dg = Da - 2;
    float* row = s.obs + w * ((long long)n_adv * Da + (long long)G * Dg);
#pragma unroll
    for (int i = 0; i < kMax; ++i) {
        if (i >= A) continue;
        float* o = i < n_adv ? row + i * Da : row + n_adv * Da + (i - n_adv) * Dg;
        int k = 0;
        o[k++] = (float)vx[i];
        o[k++] = (float)vy[i];
        o[k++] = (float)px[i];
        o[k++] = (float)py[i];
#pragma unroll
        for (int l = 0; l < ML; ++l) {
            if (l >= L) continue;
            o[k++] = (float)(lx[l] - px[i]);
            o[k++] = (float)(ly[l] - py[i]);
        }
#pragma unroll
        for (int j = 0; j < kMax; ++j) {
            if (j >= A || j == i) continue;
            o[k++] = (float)(px[j] - px[i]);
            o[k++] = (float)(py[j] - py[i]);
        }
#pragma unroll
        for (int j = 0; j < kMax; ++j) {
            if (j < n_adv || j >= A || j == i) continue;
            o[k++] = (float)vx[j];
            o[k++] = (float)vy[j];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// simple_world_comm (scenarios/simple_world_comm.py): simple_tag's adversaries and good agents among L obstacles that
// collide, followed in the landmark list by 2 pieces of food and 2 forests that do not.  Agent 0, the adversaries' leader,
// says one of 4 words per step (one word per world, advanced in place like simple_speaker_listener's; -1: nothing said
// since the restart) that every adversary observes.  Forests hide agents: agent i sees agent j iff i is the leader, both
// are inside the same forest, or neither is inside any.  Not collaborative; the observation leaves as ONE row per world,
// the agents' columns in agent order.
constexpr int kWcObstacles = MAPPO_WORLD_COMM_MAX_OBSTACLES, kWcFood = 2, kWcForests = 2;
constexpr int kWcFixed = kWcFood + kWcForests, kWcLandmarks = kWcObstacles + kWcFixed, kWcWords = 4;
constexpr double kWcLandmarkScale = 0.8, kWcObstacleSize = 0.2, kWcFoodSize = 0.03, kWcForestSize = 0.3;
constexpr double kWcCatch = 5.0, kWcFoodReward = 2.0;
// (adversary, good agent)
constexpr double kWcSize[2] = {0.075, 0.045}, kWcAccel[2] = {3.0, 4.0}, kWcMaxSpeed[2] = {1.0, 1.3};

struct WorldCommArgs {
    World s;                        // s.land: [N, L + 4, 2]; s.obs: [N, Nadv Da + G Dg], see the observation below
    long long* comm;                // [N] the leader's last word, -1 = nothing said
    const long long* act;           // [N, A + 1] (the leader's movement 0..4, its word 0..3, the others' movements)
    int A, n_adv, L;                // L: obstacles
};

// landmark `which` of a list whose length is known only at run time, without indexing the registers
template <int ML>
__device__ __forceinline__ void pick_landmark(int which, const double (&lx)[ML], const double (&ly)[ML], double& x,
                                              double& y) {
    x = y = 0.0;
#pragma unroll
    for (int l = 0; l < ML; ++l) {
        if (l == which) {
            x = lx[l];
            y = ly[l];
        }
    }
}

__global__ void __launch_bounds__(64) world_comm_step_kernel(WorldCommArgs a) {
    const long long w = (long long)blockIdx.x * 64 + threadIdx.x;
    const World& s = a.s;
    if (w >= s.n) return;
    const int A = a.A, L = a.L, n_adv = a.n_adv, Lt = a.L + kWcFixed;
    constexpr int ML = kWcLandmarks;
    double px[kMax], py[kMax], vx[kMax], vy[kMax], lx[ML], ly[ML];
    load_world(s, w, A, Lt, px, py, vx, vy, lx, ly);
    const ByKind size{n_adv, kWcSize[0], kWcSize[1]};
    const long long* act = a.act + w * (A + 1);
    // ---- the word becomes the communication state; forces: action (the acceleration acts twice, as in simple_tag) + soft
    // contacts with agents and with the obstacles, the first L landmarks
    long long comm = act[1];
    {
        const ByKind scale{n_adv, kWcAccel[0] * kWcAccel[0], kWcAccel[1] * kWcAccel[1]};
        double fx[kMax], fy[kMax];
#pragma unroll
        for (int i = 0; i < kMax; ++i) {
            if (i < A) action_force(act[i == 0 ? 0 : i + 1], fx[i], fy[i], scale.of(i));
        }
        add_contact_forces(A, size, px, py, fx, fy);
        add_landmark_contact_forces(A, L, size, kWcObstacleSize, px, py, lx, ly, fx, fy);
        integrate<true>(A, px, py, vx, vy, fx, fy, 0, ByKind{n_adv, kWcMaxSpeed[0], kWcMaxSpeed[1]});
    }
    long long t = s.t[w] + 1;
    // ---- reward (simple_world_comm.py:154-199).  Adversary: +5 per (good agent, adversary) pair in touch, whoever the
    // adversary, -0.1 x its distance to the nearest good agent.  Good agent: -5 per adversary that touches it, twice the
    // penalty for leaving the screen, +2 per food it touches, +0.05 x its distance to the nearest food
    {
        double pa[kMax];
#pragma unroll
        for (int i = 0; i < kMax; ++i) pa[i] = 0.0;
        int hits = 0;
#pragma unroll
        for (int j = 0; j < kMax; ++j) {
            if (j >= n_adv || j >= A) continue;
            double nearest = 1e300;
#pragma unroll
            for (int g = 0; g < kMax; ++g) {
                if (g < n_adv || g >= A) continue;
                const double dx = px[g] - px[j], dy = py[g] - py[j];
                const double d = sqrt(dx * dx + dy * dy);
                const bool touch = d < kWcSize[1] + kWcSize[0];
                hits += touch;
                if (touch) pa[g] -= kWcCatch;
                nearest = fmin(nearest, d);
            }
            pa[j] = -0.1 * nearest;
        }
        double food_x[kWcFood], food_y[kWcFood];
#pragma unroll
        for (int f = 0; f < kWcFood; ++f) pick_landmark(L + f, lx, ly, food_x[f], food_y[f]);
#pragma unroll
        for (int i = 0; i < kMax; ++i) {
            if (i >= A) continue;
            if (i < n_adv) {
                pa[i] += kWcCatch * hits;
                continue;
            }
            int fed = 0;
            double nearest = 1e300;
#pragma unroll
            for (int f = 0; f < kWcFood; ++f) {
                const double dx = px[i] - food_x[f], dy = py[i] - food_y[f];
                const double d = sqrt(dx * dx + dy * dy);
                fed += d < kWcSize[1] + kWcFoodSize;
                nearest = fmin(nearest, d);
            }
            pa[i] = pa[i] - 2 * (tag_bound(fabs(px[i])) + tag_bound(fabs(py[i]))) + kWcFoodReward * fed + 0.05 * nearest;
        }
        const bool restart = write_outcome(s, w, A, t, pa, 0.0, false);
        if (restart) {
            t = 0;
            restart_from_fresh(s, w, A, Lt, kWcLandmarkScale, px, py, vx, vy, lx, ly);
            comm = -1;
        }
        store_world(s, w, A, Lt, t, restart, px, py, vx, vy, lx, ly);
        a.comm[w] = comm;
    }
    // ---- who is inside which forest of the (possibly restarted) world (simple_world_comm.py:232-240 is_collision), one bit
    // per agent: the visibility mask and the in_forest columns both read these
    unsigned in0 = 0, in1 = 0;
    {
        double f0x, f0y, f1x, f1y;
        pick_landmark(L + kWcFood, lx, ly, f0x, f0y);
        pick_landmark(L + kWcFood + 1, lx, ly, f1x, f1y);
#pragma unroll
        for (int i = 0; i < kMax; ++i) {
            if (i >= A) continue;
            const double reach = size.of(i) + kWcForestSize;
            const double ax = px[i] - f0x, ay = py[i] - f0y, bx = px[i] - f1x, by = py[i] - f1y;
            in0 |= (unsigned)(sqrt(ax * ax + ay * ay) < reach) << i;
            in1 |= (unsigned)(sqrt(bx * bx + by * by) < reach) << i;
        }
    }
    const unsigned open = ~(in0 | in1);
    // ---- observation (simple_world_comm.py:225-288): own velocity, own position, the landmarks and the other agents
    // relative to the agent -- (0, 0) for one it does not see --, then for an adversary the good agents' velocities (masked
    // alike), its two in_forest flags as +-1 and the leader's word (one-hot); for a good agent the two flags and the other
    // good agents' velocities (masked)
    const int G = A - n_adv;
    const int Dc = 4 + 2 * Lt + 2 * (A - 1) + 2, Da = Dc + 2 * G + kWcWords, Dg = Dc + 2 * (G - 1);
    float* row = s.obs + w * ((long long)n_adv * Da + (long long)G * Dg);
#pragma unroll
    for (int i = 0; i < kMax; ++i) {
        if (i >= A) continue;
        float* o = i < n_adv ? row + i * Da : row + n_adv * Da + (i - n_adv) * Dg;
        const bool i0 = (in0 >> i) & 1u, i1 = (in1 >> i) & 1u;
        // bit j: agent i sees agent j
        const unsigned sees = i == 0 ? ~0u : (i0 ? in0 : 0u) | (i1 ? in1 : 0u) | (i0 || i1 ? 0u : open);
        int k = 0;
        o[k++] = (float)vx[i];
        o[k++] = (float)vy[i];
        o[k++] = (float)px[i];
        o[k++] = (float)py[i];
#pragma unroll
        for (int l = 0; l < ML; ++l) {
            if (l >= Lt) continue;
            o[k++] = (float)(lx[l] - px[i]);
            o[k++] = (float)(ly[l] - py[i]);
        }
#pragma unroll
        for (int j = 0; j < kMax; ++j) {
            if (j >= A || j == i) continue;
            const bool seen = (sees >> j) & 1u;
            o[k++] = seen ? (float)(px[j] - px[i]) : 0.f;
            o[k++] = seen ? (float)(py[j] - py[i]) : 0.f;
        }
        if (i >= n_adv) {
            o[k++] = i0 ? 1.f : -1.f;
            o[k++] = i1 ? 1.f : -1.f;
        }
#pragma unroll
        for (int j = 0; j < kMax; ++j) {
            if (j < n_adv || j >= A || j == i) continue;
            const bool seen = (sees >> j) & 1u;
            o[k++] = seen ? (float)vx[j] : 0.f;
            o[k++] = seen ? (float)vy[j] : 0.f;
        }
        if (i < n_adv) {
            o[k++] = i0 ? 1.f : -1.f;
            o[k++] = i1 ? 1.f : -1.f;
#pragma unroll
            for (int word = 0; word < kWcWords; ++word) o[k++] = comm == word ? 1.f : 0.f;
        }
    }
}

// one thread per world, 64 to a block
template <typename ArgsT>
int launch_step(void (*kernel)(ArgsT), const ArgsT& a, mappo_stream_t stream_) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((a.s.n + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream_), a);
    return (int)hipGetLastError();
}

long long* i64(int64_t* p) { return reinterpret_cast<long long*>(p); }
const long long* i64(const int64_t* p) { return reinterpret_cast<const long long*>(p); }

}  // namespace

extern "C" int mappo_simple_spread_step(double* pos, double* vel, double* landmarks, int64_t* t, const int64_t* actions,
                                        const double* fresh_pos, const double* fresh_landmarks, float* obs,
                                        float* rewards, uint8_t* dones, double* per_agent, int64_t n_worlds,
                                        int num_agents, int num_landmarks, int world_length, int auto_reset,
                                        mappo_stream_t stream_) {
    if (!pos || !vel || !landmarks || !t || !actions || !obs || !rewards || !dones || !per_agent) return MAPPO_E_NULL;
    if (auto_reset && (!fresh_pos || !fresh_landmarks)) return MAPPO_E_NULL;
    if (n_worlds <= 0 || num_agents < 1 || num_landmarks < 1 || world_length < 1) return MAPPO_E_SHAPE;
    if (num_agents > kMax || num_landmarks > kMax) return MAPPO_E_TOO_MANY;
    const World s{pos, vel, landmarks, i64(t), fresh_pos, fresh_landmarks, obs, rewards, dones, per_agent,
                  n_worlds, world_length, auto_reset};
    return launch_step(spread_step_kernel, Args{s, i64(actions), num_agents, num_landmarks}, stream_);
}

extern "C" int mappo_simple_reference_step(double* pos, double* vel, double* landmarks, int64_t* t, int64_t* goals,
                                           int64_t* comm, const int64_t* actions, const double* fresh_pos,
                                           const double* fresh_landmarks, const int64_t* fresh_goals, float* obs,
                                           float* rewards, uint8_t* dones, double* per_agent, int64_t n_worlds,
                                           int world_length, int auto_reset, mappo_stream_t stream_) {
    if (!pos || !vel || !landmarks || !t || !goals || !comm || !actions || !obs || !rewards || !dones || !per_agent)
        return MAPPO_E_NULL;
    if (auto_reset && (!fresh_pos || !fresh_landmarks || !fresh_goals)) return MAPPO_E_NULL;
    if (n_worlds <= 0 || world_length < 1) return MAPPO_E_SHAPE;
    const World s{pos, vel, landmarks, i64(t), fresh_pos, fresh_landmarks, obs, rewards, dones, per_agent,
                  n_worlds, world_length, auto_reset};
    return launch_step(reference_step_kernel, RefArgs{s, i64(goals), i64(comm), i64(actions), i64(fresh_goals)},
                       stream_);
}

extern "C" int mappo_simple_speaker_listener_step(double* pos, double* vel, double* landmarks, int64_t* t, int64_t* goal,
                                                  int64_t* comm, const int64_t* actions, const double* fresh_pos,
                                                  const double* fresh_landmarks, const int64_t* fresh_goal, float* obs,
                                                  float* rewards, uint8_t* dones, double* per_agent, int64_t n_worlds,
                                                  int world_length, int auto_reset, mappo_stream_t stream_) {
    if (!pos || !vel || !landmarks || !t || !goal || !comm || !actions || !obs || !rewards || !dones || !per_agent)
        return MAPPO_E_NULL;
    if (auto_reset && (!fresh_pos || !fresh_landmarks || !fresh_goal)) return MAPPO_E_NULL;
    if (n_worlds <= 0 || world_length < 1) return MAPPO_E_SHAPE;
    const World s{pos, vel, landmarks, i64(t), fresh_pos, fresh_landmarks, obs, rewards, dones, per_agent,
                  n_worlds, world_length, auto_reset};
    return launch_step(speaker_listener_step_kernel,
                       SpeakerArgs{s, i64(goal), i64(comm), i64(actions), i64(fresh_goal)}, stream_);
}

extern "C" int mappo_simple_push_step(double* pos, double* vel, double* landmarks, int64_t* t, int64_t* goal,
                                      const int64_t* actions, const double* fresh_pos, const double* fresh_landmarks,
                                      const int64_t* fresh_goal, float* obs, float* rewards, uint8_t* dones,
                                      double* per_agent, int64_t n_worlds, int num_agents, int num_landmarks,
                                      int world_length, int auto_reset, mappo_stream_t stream_) {
    if (!pos || !vel || !landmarks || !t || !goal || !actions || !obs || !rewards || !dones || !per_agent)
        return MAPPO_E_NULL;
    if (auto_reset && (!fresh_pos || !fresh_landmarks || !fresh_goal)) return MAPPO_E_NULL;
    if (n_worlds <= 0 || num_agents < 2 || num_landmarks < 1 || num_landmarks > kPushLandmarks || world_length < 1)
        return MAPPO_E_SHAPE;
    if (num_agents > kMax) return MAPPO_E_TOO_MANY;
    const World s{pos, vel, landmarks, i64(t), fresh_pos, fresh_landmarks, obs, rewards, dones, per_agent,
                  n_worlds, world_length, auto_reset};
    return launch_step(push_step_kernel, PushArgs{s, i64(goal), i64(actions), i64(fresh_goal), num_agents, num_landmarks},
                       stream_);
}

extern "C" int mappo_simple_tag_step(double* pos, double* vel, double* landmarks, int64_t* t, const int64_t* actions,
                                     const double* fresh_pos, const double* fresh_landmarks, float* obs, float* rewards,
                                     uint8_t* dones, double* per_agent, int64_t n_worlds, int num_agents,
                                     int num_adversaries, int num_landmarks, int world_length, int auto_reset,
                                     mappo_stream_t stream_) {
    if (!pos || !vel || !landmarks || !t || !actions || !obs || !rewards || !dones || !per_agent) return MAPPO_E_NULL;
    if (auto_reset && (!fresh_pos || !fresh_landmarks)) return MAPPO_E_NULL;
    if (n_worlds <= 0 || num_adversaries < 1 || num_adversaries >= num_agents || num_landmarks < 1 || world_length < 1)
        return MAPPO_E_SHAPE;
    if (num_agents > kMax || num_landmarks > kTagLandmarks) return MAPPO_E_TOO_MANY;
    const World s{pos, vel, landmarks, i64(t), fresh_pos, fresh_landmarks, obs, rewards, dones, per_agent,
                  n_worlds, world_length, auto_reset};
    return launch_step(tag_step_kernel, TagArgs{s, i64(actions), num_agents, num_adversaries, num_landmarks}, stream_);
}

extern "C" int mappo_simple_world_comm_step(double* pos, double* vel, double* landmarks, int64_t* t, int64_t* comm,
                                            const int64_t* actions, const double* fresh_pos,
                                            const double* fresh_landmarks, float* obs, float* rewards, uint8_t* dones,
                                            double* per_agent, int64_t n_worlds, int num_agents, int num_adversaries,
                                            int num_landmarks, int world_length, int auto_reset,
                                            mappo_stream_t stream_) {
    if (!pos || !vel || !landmarks || !t || !comm || !actions || !obs || !rewards || !dones || !per_agent)
        return MAPPO_E_NULL;
    if (auto_reset && (!fresh_pos || !fresh_landmarks)) return MAPPO_E_NULL;
    if (n_worlds <= 0 || num_adversaries < 1 || num_adversaries >= num_agents || num_landmarks < 1 || world_length < 1)
        return MAPPO_E_SHAPE;
    if (num_agents > kMax || num_landmarks > kWcObstacles) return MAPPO_E_TOO_MANY;
    const World s{pos, vel, landmarks, i64(t), fresh_pos, fresh_landmarks, obs, rewards, dones, per_agent,
                  n_worlds, world_length, auto_reset};
    return launch_step(world_comm_step_kernel,
                       WorldCommArgs{s, i64(comm), i64(actions), num_agents, num_adversaries, num_landmarks}, stream_);
}
