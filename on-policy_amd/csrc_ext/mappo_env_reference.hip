// K11 family: one step of all simple_reference worlds as ONE launch (reference onpolicy/envs/mpe/scenarios/
// simple_reference.py goals / reward / observation, environment.py:115-255 MultiDiscrete decoding, core.py:207-288
// integration and communication state).  Two agents, three landmarks, no contact forces: the per-world work is a few
// dozen float64 operations, so as in K11's spread_step_kernel (csrc/mappo_env.hip) a thread owns a world and keeps it in
// registers.  The state a replayed graph carries -- pos, vel, landmarks, t, the goal landmark of each agent, the index of
// each agent's last communication symbol (-1: silent) -- is advanced in place; restarted worlds take fresh_* (drawn for
// every world by the caller, used where a world restarts), so the trajectories are those of
// envs/mpe/simple_reference.py::_step_ops.
#include <hip/hip_runtime.h>

#include "../../include/mappo_hip.h"
#include "../csrc/mappo_internal.h"

namespace {

// the physics constants of K11 (csrc/mappo_env.hip)
constexpr double kDt = 0.1, kDamping = 0.25, kSens = 5.0;
constexpr int kRefAgents = 2, kRefLandmarks = 3, kRefSymbols = 10;
constexpr int kRefObs = 2 + 2 * kRefLandmarks + 3 + kRefSymbols;     // 21
constexpr double kRefLandmarkScale = 0.8;

struct RefArgs {
    double* pos;                // [N, 2, 2]
    double* vel;                // [N, 2, 2]
    double* land;               // [N, 3, 2]
    long long* t;               // [N]
    long long* goal;            // [N, 2] goal landmark of each agent, 0..2
    long long* comm;            // [N, 2] last symbol of each agent, -1 = silent
    const long long* act;       // [N, 2, 2] (movement 0..4, symbol 0..9)
    const double* fresh_pos;    // [N, 2, 2] uniform(-1, 1)
    const double* fresh_land;   // [N, 3, 2] uniform(-1, 1), scaled by 0.8 here
    const long long* fresh_goal;    // [N, 2] 0..2
    float* obs;                 // [N, 2, 21]
    float* rew;                 // [N, 2, 1]
    unsigned char* done;        // [N, 2] (bool)
    double* per_agent;          // [N, 2]
    long long n;
    int world_length, auto_reset;
};

__global__ void __launch_bounds__(64) reference_step_kernel(RefArgs a) {
    const long long w = (long long)blockIdx.x * 64 + threadIdx.x;
    if (w >= a.n) return;
    double px[kRefAgents], py[kRefAgents], vx[kRefAgents], vy[kRefAgents], lx[kRefLandmarks], ly[kRefLandmarks];
    long long goal[kRefAgents], comm[kRefAgents];
#pragma unroll
    for (int i = 0; i < kRefAgents; ++i) {
        const long long k = (w * kRefAgents + i) * 2;
        px[i] = a.pos[k];
        py[i] = a.pos[k + 1];
        vx[i] = a.vel[k];
        vy[i] = a.vel[k + 1];
        goal[i] = a.goal[w * kRefAgents + i];
    }
#pragma unroll
    for (int l = 0; l < kRefLandmarks; ++l) {
        lx[l] = a.land[(w * kRefLandmarks + l) * 2];
        ly[l] = a.land[(w * kRefLandmarks + l) * 2 + 1];
    }
    // ---- action force (environment.py: u[0] += a[1] - a[2], u[1] += a[3] - a[4], x sensitivity), integration
    // (core.py: damping, then force * dt; no contacts in this scenario); the symbol becomes the communication state
#pragma unroll
    for (int i = 0; i < kRefAgents; ++i) {
        const long long mv = a.act[(w * kRefAgents + i) * 2];
        comm[i] = a.act[(w * kRefAgents + i) * 2 + 1];
        const double fx = (mv == 1 ? 1.0 : mv == 2 ? -1.0 : 0.0) * kSens;
        const double fy = (mv == 3 ? 1.0 : mv == 4 ? -1.0 : 0.0) * kSens;
        vx[i] = vx[i] * (1 - kDamping) + fx * kDt;
        vy[i] = vy[i] * (1 - kDamping) + fy * kDt;
        px[i] = px[i] + vx[i] * kDt;
        py[i] = py[i] + vy[i] * kDt;
    }
    long long t = a.t[w] + 1;
    // ---- reward (simple_reference.py: -|goal_a - goal_b|^2, goal_a = the other agent), shared as r_0 + r_1
    double pa[kRefAgents];
#pragma unroll
    for (int i = 0; i < kRefAgents; ++i) {
        const int o = kRefAgents - 1 - i;
        const long long g = goal[i];
        const double gx = g == 0 ? lx[0] : g == 1 ? lx[1] : lx[2];
        const double gy = g == 0 ? ly[0] : g == 1 ? ly[1] : ly[2];
        const double dx = px[o] - gx, dy = py[o] - gy;
        pa[i] = -(dx * dx + dy * dy);
    }
    const double total = pa[0] + pa[1];
    const bool done = t >= a.world_length;
#pragma unroll
    for (int i = 0; i < kRefAgents; ++i) {
        a.per_agent[w * kRefAgents + i] = pa[i];
        a.rew[w * kRefAgents + i] = (float)total;
        a.done[w * kRefAgents + i] = done ? 1 : 0;
    }
    const bool restart = done && a.auto_reset;
    if (restart) {
        t = 0;
#pragma unroll
        for (int i = 0; i < kRefAgents; ++i) {
            const long long k = (w * kRefAgents + i) * 2;
            px[i] = a.fresh_pos[k];
            py[i] = a.fresh_pos[k + 1];
            vx[i] = 0.0;
            vy[i] = 0.0;
            goal[i] = a.fresh_goal[w * kRefAgents + i];
            comm[i] = -1;
        }
#pragma unroll
        for (int l = 0; l < kRefLandmarks; ++l) {
            lx[l] = kRefLandmarkScale * a.fresh_land[(w * kRefLandmarks + l) * 2];
            ly[l] = kRefLandmarkScale * a.fresh_land[(w * kRefLandmarks + l) * 2 + 1];
        }
    }
    a.t[w] = t;
#pragma unroll
    for (int i = 0; i < kRefAgents; ++i) {
        const long long k = (w * kRefAgents + i) * 2;
        a.pos[k] = px[i];
        a.pos[k + 1] = py[i];
        a.vel[k] = vx[i];
        a.vel[k + 1] = vy[i];
        a.comm[w * kRefAgents + i] = comm[i];
        if (restart) a.goal[w * kRefAgents + i] = goal[i];
    }
    if (restart) {
#pragma unroll
        for (int l = 0; l < kRefLandmarks; ++l) {
            a.land[(w * kRefLandmarks + l) * 2] = lx[l];
            a.land[(w * kRefLandmarks + l) * 2 + 1] = ly[l];
        }
    }
    // ---- observation of the (possibly restarted) world (simple_reference.py observation): own velocity, landmarks
    // relative to the agent, the colour of the agent's goal landmark, the other agent's communication state (one-hot)
#pragma unroll
    for (int i = 0; i < kRefAgents; ++i) {
        float* o = a.obs + (w * kRefAgents + i) * kRefObs;
        int k = 0;
        o[k++] = (float)vx[i];
        o[k++] = (float)vy[i];
#pragma unroll
        for (int l = 0; l < kRefLandmarks; ++l) {
            o[k++] = (float)(lx[l] - px[i]);
            o[k++] = (float)(ly[l] - py[i]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) o[k++] = goal[i] == c ? 0.75f : 0.25f;     // palette: 0.75 on the landmark's own channel
        const long long heard = comm[kRefAgents - 1 - i];
#pragma unroll
        for (int s = 0; s < kRefSymbols; ++s) o[k++] = heard == s ? 1.f : 0.f;
    }
}

}  // namespace

extern "C" int mappo_simple_reference_step(double* pos, double* vel, double* landmarks, int64_t* t, int64_t* goals,
                                           int64_t* comm, const int64_t* actions, const double* fresh_pos,
                                           const double* fresh_landmarks, const int64_t* fresh_goals, float* obs,
                                           float* rewards, uint8_t* dones, double* per_agent, int64_t n_worlds,
                                           int world_length, int auto_reset, mappo_stream_t stream_) {
    if (!pos || !vel || !landmarks || !t || !goals || !comm || !actions || !obs || !rewards || !dones || !per_agent)
        return MAPPO_E_NULL;
    if (auto_reset && (!fresh_pos || !fresh_landmarks || !fresh_goals)) return MAPPO_E_NULL;
    if (n_worlds <= 0 || world_length < 1) return MAPPO_E_SHAPE;
    RefArgs a;
    a.pos = pos;
    a.vel = vel;
    a.land = landmarks;
    a.t = reinterpret_cast<long long*>(t);
    a.goal = reinterpret_cast<long long*>(goals);
    a.comm = reinterpret_cast<long long*>(comm);
    a.act = reinterpret_cast<const long long*>(actions);
    a.fresh_pos = fresh_pos;
    a.fresh_land = fresh_landmarks;
    a.fresh_goal = reinterpret_cast<const long long*>(fresh_goals);
    a.obs = obs;
    a.rew = rewards;
    a.done = dones;
    a.per_agent = per_agent;
    a.n = n_worlds;
    a.world_length = world_length;
    a.auto_reset = auto_reset;
    hipLaunchKernelGGL(reference_step_kernel, dim3((unsigned)((n_worlds + 63) / 64)), dim3(64), 0,
                       static_cast<hipStream_t>(stream_), a);
    return (int)hipGetLastError();
}
