/*
 * rmx.h — C ABI of the MI355X-native multi-agent grid-world + Reward-Machine step engine.
 *
 * Drop-in boundary for the reference hot path (paths relative to Alee08/multiagent-rl-rm):
 *   RMEnvironmentWrapper.reset / .step / .check_terminations
 *       multiagent_rlrm/multi_agent/wrappers/rm_environment_wrapper.py:28-41, 43-107, 109-120
 *   MultiAgentFrozenLake.reset / .step / check_terminations / apply_action / holes_in_the_ice
 *       multiagent_rlrm/environments/frozen_lake/ma_frozen_lake.py:43-94, 96-154, 174-242
 *   MultiAgentOfficeWorld.reset / .step / check_terminations / apply_action / apply_wall_penalty
 *       multiagent_rlrm/environments/office_world/ma_office.py:77-120, 122-202, 204-325
 *   can_move_{up,down,left,right}      multiagent_rlrm/environments/office_world/config_office.py:12-39
 *   PositionEventDetector.detect_event multiagent_rlrm/environments/frozen_lake/detect_event.py:18-33
 *   RewardMachine.step                 multiagent_rlrm/multi_agent/reward_machine.py:45-59
 *
 * The reference's per-object Python calls become batched calls over N environments x A agents whose
 * state lives in caller-owned device buffers (structure of arrays, agent-major: column[a * N + e]).
 * All device work is enqueued on the caller's HIP stream; only rmx_stats_host / rmx_check_errors
 * synchronise.  Every entry point returns 0 on success or a negative RMX_E* code; the message is
 * available from rmx_last_error() (thread-local).
 *
 * Semantics are restated, not copied; see DESIGN.md for the rule list.
 *
 * Host handles: rmx_create with cfg.device == RMX_DEVICE_HOST steps the envs on the CPU (csrc/rmx_hoststep.cpp, over
 * the same compiled tables and rules as the generic gfx950 kernels): every entry point below then takes HOST pointers
 * wherever it says "device" (buffers, actions, masks, statistics, traces), ignores the stream and completes before it
 * returns.  It is the reference's own CPU case (BASELINE config 1: one env behind the per-call dict API) without a GPU
 * or a PCIe round trip per call.  rmx_step_variant reports RMX_VARIANT_HOST; rmx_step_seq, RMX_SEQ_HOST.
 * A host handle keeps the device's table limit: tables whose generic-kernel blob would exceed 64 KiB of LDS are refused
 * by rmx_create on either path (RMX_E_INVALID, "tables exceed 64 KiB ..."), so a config that a host handle steps is one
 * a device handle steps too.
 */
#ifndef RMX_H
#define RMX_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMX_ABI_VERSION 12

/* ---- limits (tables are staged whole into LDS per workgroup) ---------------------------------- */
#define RMX_MAX_AGENTS 8
#define RMX_MAX_CELLS 4096  /* W*H */
#define RMX_MAX_RM_STATES 255
#define RMX_MAX_EVENTS 255  /* including event 0 = "no event" (detect_event -> None) */

/* ---- error codes ---------------------------------------------------------------------------- */
#define RMX_OK 0
#define RMX_E_INVALID (-1)  /* bad argument / config            -> ValueError in Python  */
#define RMX_E_HIP (-2)      /* HIP runtime error                 -> RuntimeError          */
#define RMX_E_ACTION (-3)   /* an action outside [0,4] was seen  -> ValueError            */
#define RMX_E_STATE (-4)    /* buffers not bound / wrong sizes   -> RuntimeError          */
#define RMX_E_TRACE (-5)    /* a Q(lambda) trace list was full   -> RuntimeError          */
#define RMX_E_MODEL (-6)    /* an R-max successor list was full  -> RuntimeError          */

#define RMX_DEVICE_HOST (-1) /* rmx_config.device: the host path (no GPU) */

/* ---- environment kinds ---------------------------------------------------------------------- */
#define RMX_FROZEN_LAKE 0  /* ma_frozen_lake.py: up = y-1, RM-final agents freeze, trunc => term */
#define RMX_OFFICE_WORLD 1 /* ma_office.py:      up = y+1, walls, plants, RM-final agents keep moving */

/* ---- actions: index order of action_encoder_frozen_lake.py:14-17 / action_encoder_office_world.py:10-13 */
#define RMX_UP 0
#define RMX_DOWN 1
#define RMX_LEFT 2
#define RMX_RIGHT 3
#define RMX_WAIT 4 /* ActionRL("wait"): no move, no wall collision */

/* ---- per-cell tile bits ----------------------------------------------------------------------- */
#define RMX_CELL_CAN_UP 0x01u    /* can_move_up    (boundary, and walls for OfficeWorld) */
#define RMX_CELL_CAN_DOWN 0x02u  /* can_move_down  */
#define RMX_CELL_CAN_LEFT 0x04u  /* can_move_left  */
#define RMX_CELL_CAN_RIGHT 0x08u /* can_move_right */
#define RMX_CELL_HAZARD 0x10u    /* FrozenLake hole / OfficeWorld plant */

/* ---- per-(env, agent) flags word ------------------------------------------------------------ */
#define RMX_F_ACTIVE 0x01u   /* env.active_agents[name]                                  */
#define RMX_F_FAIL 0x02u     /* env.agent_fail[name]                                     */
#define RMX_F_TERM 0x04u     /* wrapper terminations[name] (env OR RM) after this step   */
#define RMX_F_TRUNC 0x08u    /* wrapper truncations[name]                                */
#define RMX_F_ENV_TERM 0x10u /* infos[name]["env_terminated"]                            */
#define RMX_F_RM_TERM 0x20u  /* infos[name]["rm_terminated"]                             */
#define RMX_F_ENV_DONE 0x40u /* the episode of this env ended at this step (loop rule)   */
#define RMX_F_STEPS_SHIFT 16 /* bits 16..31: env.agent_steps[name]                       */

/* ---- statistics vector (rmx_stats_*): sums over finished episodes ------------------------- */
#define RMX_STAT_SUM_RETURN 0 /* sum over (env-episode, agent) of the episode return           */
#define RMX_STAT_EPISODES 1   /* number of finished env-episodes                                */
#define RMX_STAT_SUCCESSES 2  /* number of (env-episode, agent) successes (evaluation_metrics.py:248-267) */
#define RMX_STAT_SUM_LENGTH 3 /* sum over env-episodes of env.timestep at the end               */
#define RMX_NSTATS 4

typedef struct rmx_config {
  int32_t kind;        /* RMX_FROZEN_LAKE or RMX_OFFICE_WORLD                                   */
  int32_t width;       /* grid_width  (W)                                                       */
  int32_t height;      /* grid_height (H)                                                       */
  int32_t n_agents;    /* A, 1..RMX_MAX_AGENTS                                                  */
  int32_t n_rm_states; /* Q: row count of the dense RM tables (max over agents)                 */
  int32_t n_events;    /* E: 1 + number of distinct event cells (event 0 = None)                */
  int32_t max_t;       /* truncation when timestep > max_t (1000 in the reference)              */
  int32_t device;      /* HIP device ordinal the handle binds to, or RMX_DEVICE_HOST            */
  int64_t n_envs;      /* N: envs in THIS shard (one rank / GPU)                                */
  int64_t env_offset;  /* global index of env 0 of this shard (action hash, sharding)           */
  int64_t n_envs_global; /* N over all shards (action hash)                                     */
  float hazard_penalty;  /* FL penalty_amount / OW plants_penalty_value                         */
  float wall_penalty;    /* OW wall_penalty_value (ignored for FL: a boundary block is free)     */
  int32_t hazard_fail;   /* FL: 1 (holes always fail) / OW: terminate_on_plants                  */
  int32_t wall_fail;     /* OW: terminate_hit_walls                                              */
  float gamma;           /* episode-return discount for the stats (OW loop: gamma, FL loop: 1.0) */
  int32_t has_shaping;   /* 1 if shape[] is given (potential-based shaping column)               */
  float reward_modifier; /* RMEnvironmentWrapper.reward_modifier (rm_environment_wrapper.py:26,69) */
  int32_t n_qrm_max;     /* Qx: max over agents of len(get_all_states()) - 1 (QRM experiences)    */
  /* Stochastic slip (ma_frozen_lake.py:244-298, ma_office.py:327-379): numpy Generator(PCG64) per env,
   * seeded by SeedSequence(seed) at every reset (default_rng(seed)), one rng.choice draw per agent that
   * actually slips, in agent order.  seed of env e (global index) in its k-th episode since rmx_reset:
   *   seed = base_seed * seed_scale + e * seed_env_stride + k * seed_episode_stride   (mod 2^64)
   * (FrozenLake runner: reset(args.seed) every episode; OfficeWorld runner: reset(seed*1000 + episode)). */
  int32_t stochastic;           /* 0: deterministic dynamics; 1: slip tables below are used           */
  int32_t slip_n[4];            /* outcomes per intended action (<= 4)                               */
  int32_t slip_out[4][4];       /* outcome action ids (RMX_UP..RMX_WAIT) in the reference's list order */
  double slip_cdf[4][4];        /* p.cumsum() / p.cumsum()[-1] exactly as Generator.choice computes it */
  uint64_t seed_scale, seed_env_stride, seed_episode_stride;
  /* FrozenLake random_start_positions (ma_frozen_lake.py:37-39, 59-64, 156-172): at every reset the agents
   * start on the first A cells of the non-hole cells in x-major order ((x, y) for x in range(W) for y in
   * range(H)) shuffled by numpy Generator.shuffle with the env rng just seeded for that episode, i.e. BEFORE
   * any slip draw of the episode.  Needs the rng / episode buffers like stochastic mode (the same seed
   * schedule); start_xy is then unused.  FrozenLake only; at least A non-hole cells. */
  int32_t random_starts;
  /* host pointers, copied at rmx_create */
  const uint16_t* cell;       /* [H*W]       RMX_CELL_* bits, index y*W + x                   */
  const uint8_t* cell_event;  /* [A][H*W]    event id 0..E-1 detected at that cell per agent    */
  const uint8_t* next_q;      /* [A][Q][E]   RM successor; missing (q,e) => q (self loop)       */
  const float* rm_reward;     /* [A][Q][E]   RM transition reward (raw); missing => 0           */
  const float* shape;         /* [A][Q][E]   gamma*Phi(next_q) - Phi(q), or NULL                */
  const int32_t* init_q;      /* [A]         RM initial-state index (always 0 in the reference) */
  const int32_t* final_q;     /* [A]         RM final-state index (last inserted to_state)      */
  const int32_t* start_xy;    /* [A][2]      initial (x, y) per agent                           */
  /* QRM counterfactual experiences (rm_environment_wrapper.py:122-183); may be NULL if n_qrm_max == 0 */
  const int32_t* n_qrm;       /* [A]         len(rm.get_all_states()) - 1                        */
  const uint8_t* qrm_states;  /* [A][Qx]     RM-state indices in get_all_states() order (last dropped) */
  const int32_t* enc_nq;      /* [A]         rm.numbers_state() (state encoder stride, state_encoder_*.py) */
} rmx_config;

/* Caller-owned device buffers; columns are agent-major [A][N] (index a*N + e). */
typedef struct rmx_buffers {
  int32_t* pos_x;    /* [A][N] state  */
  int32_t* pos_y;    /* [A][N] state  */
  int32_t* rm_q;     /* [A][N] state: RM state index (RewardMachine.get_state_index)      */
  uint32_t* flags;   /* [A][N] state: RMX_F_* bits + agent_steps                          */
  float* ep_ret;     /* [A][N] state: running episode return (FL sum, OW discounted sum)   */
  int32_t* t;        /* [N]    state: env.timestep                                       */
  float* reward;     /* [A][N] out:   wrapper rewards[name] = Renv + reward_modifier * RQ  */
  float* shaping;    /* [A][N] out:   gamma*Phi(q') - Phi(q) (NULL: not written)          */
  uint8_t* env_done; /* [N]    out:   1 where the episode ended this step (NULL: not written) */
  float* renv;       /* [A][N] out:   infos["Renv"] (NULL: not written)                   */
  /* QRM experiences, [A][Qx][N] each (NULL: not computed).  Experience j of agent a is
   * (qrm_s, action, Renv + qrm_rq, qrm_sn, qrm_done, qrm_s / nQ, qrm_s % nQ, qrm_sn / nQ, qrm_sn % nQ,
   * qrm_rq) of rm_environment_wrapper.py:168-179, nQ = enc_nq[a]. */
  int32_t* qrm_s;    /* encoder.encode(prev position, state j)                       */
  int32_t* qrm_sn;   /* encoder.encode(new position, hypothetical next state)        */
  float* qrm_rq;     /* hypothetical RM reward (raw, not scaled by reward_modifier)  */
  uint8_t* qrm_done; /* env termination OR hypothetical next state == final          */
  /* required when cfg.stochastic or cfg.random_starts: per-env PCG64 state and episode counter */
  uint64_t* rng;     /* [4][N] state_hi, state_lo, inc_hi, inc_lo (128-bit LCG of numpy's PCG64) */
  int32_t* episode;  /* [N]    episodes started since rmx_reset (the k of the seed schedule)      */
  /* optional learner input (NULL: not written): the post-step observation encoded as the reference's
   * state encoders do, (pos_y * W + pos_x) * enc_nq[a] + rm_q (state_encoder_frozen_lake.py:23-35,
   * state_encoder_office.py:15-24).  Needs cfg.enc_nq. */
  int32_t* enc_state; /* [A][N] */
} rmx_buffers;

typedef struct rmx_handle rmx_handle;

/* Version / diagnostics */
int rmx_abi_version(void);
/* HIP devices visible to this process (0 without a driver or a device: host handles still work); no reference
 * counterpart (the reference runs on the CPU only). */
int rmx_device_count(int32_t* n);
const char* rmx_last_error(void);
/* Build provenance (no reference counterpart): "src=<first 16 hex digits of the SHA-256 of the engine
 * sources, in the Makefile's RMX_HASHED order> kern=<the same of the fast kernels' gfx950 code object>
 * abi=<RMX_ABI_VERSION> arch=<offload arch>".  A loader compares src with the sources it ships to refuse a stale
 * library; kern ties a kernel profile to the machine code it measured. */
const char* rmx_build_info(void);

/* Create a handle: validates the config, uploads tables to the device, allocates the stats slab.
 * Replaces the object graph built by frozen_lake_main.py:199-267 / office_main.py:400-605. */
int rmx_create(const rmx_config* cfg, rmx_handle** out);
void rmx_destroy(rmx_handle* h);

/* Bind caller-owned device buffers (sizes implied by cfg.n_envs and cfg.n_agents). */
int rmx_bind(rmx_handle* h, const rmx_buffers* buf);

/* RMEnvironmentWrapper.reset (rm_environment_wrapper.py:28-41) for the envs whose env_mask byte is
 * nonzero (all envs if env_mask == NULL): timestep 0, agents active at their start cells, RM at its
 * initial state, episode return 0.  `seed` becomes the base seed of the schedule above; stochastic mode
 * reseeds each reset env with episode k = 0 (deterministic dynamics ignore it). */
int rmx_reset(rmx_handle* h, const uint8_t* env_mask_dev, uint64_t seed, void* hip_stream);

/* One RMEnvironmentWrapper.step (rm_environment_wrapper.py:43-107) for every env of the shard.
 * actions_dev: int32 [A][N] device array (RMX_UP..RMX_WAIT).  If autoreset != 0, envs whose previous
 * step ended their episode (RMX_F_ENV_DONE) are reset first, mirroring the reference loops
 * (frozen_lake_main.py:336-376, office_main.py:1696-1749), then stepped with this action. */
int rmx_step(rmx_handle* h, const int32_t* actions_dev, int autoreset, void* hip_stream);

/* As rmx_step, with actions generated in-kernel by the SURVEY §8(d) counter hash
 * a = splitmix64(seed ^ (((t_global*N_global + e_global)*A + i) * 0x9E3779B97F4A7C15)) >> 62. */
int rmx_step_hashed(rmx_handle* h, uint64_t seed, int64_t t_global, int autoreset, void* hip_stream);

/* Fill actions_dev[T][A][N] with the same hash for global steps t0 .. t0+T-1 (test / bench input). */
int rmx_fill_actions(rmx_handle* h, uint64_t seed, int64_t t0, int32_t T, int32_t* actions_dev,
                     void* hip_stream);

/* Fused rollout: T autoreset steps with hashed actions, state kept in registers, per-episode stats
 * accumulated; state columns written back once at the end.  reward_trace_dev (optional, NULL = off)
 * receives float [T][A][N] rewards. */
int rmx_rollout(rmx_handle* h, uint64_t seed, int64_t t0, int32_t T, float* reward_trace_dev,
                void* hip_stream);

/* RMEnvironmentWrapper.get_mdp (rm_environment_wrapper.py:185-283) for one agent, deterministic dynamics:
 * S = W*H*enc_nq[agent] encoded states (rmx_mdp_states); outputs [S][4] device arrays: next encoded state
 * (-1 = no entry), reward, done (0/1, 255 = no entry).  Terminal states (hole / plant with
 * terminate_on_plants / RM final) self-loop.  fix_frozen_lake = 0 reproduces the reference exactly,
 * including its FrozenLake quirk (decode returns {"q": label}, so non-hole FL states get no entries);
 * 1 decodes the RM index as the OfficeWorld encoder does. Needs no bound buffers. */
int rmx_mdp_states(rmx_handle* h, int32_t agent, int64_t* n_states);
int rmx_mdp(rmx_handle* h, int32_t agent, int32_t fix_frozen_lake, int32_t* next_dev, float* reward_dev,
            uint8_t* done_dev, void* hip_stream);

/* Episode statistics accumulated since the last rmx_stats_clear (RMX_NSTATS doubles).
 * _device writes them to a device buffer (for an RCCL all-reduce), _host synchronises. */
int rmx_stats_device(rmx_handle* h, double* out_dev, void* hip_stream);
int rmx_stats_host(rmx_handle* h, double* out_host);
int rmx_stats_clear(rmx_handle* h, void* hip_stream);

/* rmx_step followed by rmx_stats_device(stats_out_dev) on the same stream: the step of a loop iteration that
 * also logs the episode statistics (frozen_lake_main.py:368-376, office_main.py:1743-1749; the vector an
 * RCCL all-reduce then sums across ranks).  Where the handle runs the default thread-per-env fast kernel
 * below 1M envs on deterministic dynamics, the report is computed inside the step launch (one launch instead of
 * two); slip handles, QRM-bound, lane-per-agent and per-wave-statistics (>= 1M envs) handles and the generic
 * kernels take the two launches.  Integer statistics are identical either way; the fused report's return sum is a
 * fixed-order sum with its own association, so it may differ from rmx_stats_device's in the last bits.
 * Like rmx_stats_device it uses the handle's reduction scratch: one report in flight per handle (calls on one
 * stream, as everything else on a handle).
 * rmx_step_report_fused: 1 if this (bound) handle fuses the report, else 0 (no device work). */
int rmx_step_report(rmx_handle* h, const int32_t* actions_dev, int autoreset, double* stats_out_dev,
                    void* hip_stream);
int rmx_step_report_fused(const rmx_handle* h);

/* n_steps iterations of the reference loops' inner step (frozen_lake_main.py:336-376, office_main.py:1696-1749) in
 * one submission: step k is rmx_step with actions_dev + k * action_stride (int32 elements, each an [A][N] array as
 * for rmx_step); with stats_out_dev != NULL the last one is rmx_step_report's (the statistics vector written
 * there).  Results identical to those n_steps calls on hip_stream.  BLOCKING: returns once the steps are complete
 * on the device (work enqueued on hip_stream before the call runs first).  Where the handle's step is the
 * thread-per-env fast kernel the launches go to the engine's own AQL queue on the device (one per device, K
 * kernel-dispatch packets and one doorbell: no per-launch runtime work); elsewhere they are the calls on hip_stream,
 * then a stream synchronisation.  1 <= n_steps <= 2^20.
 * The stream path also serves a fast handle whenever the queue cannot: RMX_QUEUE=0 in the environment at rmx_create,
 * a queue that could not be set up on the device (no HSA agent found for it, a loader error), a step kernel the queue
 * refuses (its code-object metadata lists a hidden argument the queue does not write, e.g. a debugging printf's), and
 * every window after a failed one.  A window fails (RMX_E_HIP, its results undefined) when the queue faults or does
 * not complete within 60 s; the queue is then inactivated (none of its packets keeps running) and retired for the
 * process.
 * Inside a queue window the steps may hand the state to each other in a private layout of the handle's own and skip
 * outputs that a later step of the same window overwrites (reward, env_done and the optional per-step columns of
 * every step but the last): the caller's buffers are read by the window's first step and written by its last, and
 * hold after the call exactly what the n_steps calls would have left.  A failed window leaves them undefined, as
 * before.  The default deterministic step (no slip, fixed starts, no QRM outputs, below 1M envs) takes this form for
 * n_steps >= 2; RMX_SEQ_PACKED=0 in the environment at rmx_create keeps the window of n_steps column-to-column steps.
 * Fences: every packet of a window waits for the one before it (barrier bit) and starts with an agent-scope acquire.
 * The packets of a packed window before its last end with NO release fence: all they leave behind is the handle's
 * private record and its statistics slots, written with write-through stores and agent-scope atomics that each wave
 * waits for before it ends.  The last packet of a packed window, every packet of an unpacked one and a window of one
 * step end with an agent-scope release.  RMX_SEQ_RELEASE=1 in the environment at rmx_create keeps the release on
 * every packet (results are the same; the switch is for measurements and as a fallback).
 * rmx_seq_handoff(k, n_steps, packed, release_all): 1 if packet k of an n_steps window is recorded as such a private
 * hand-off (no release fence), for a packed / unpacked window and RMX_SEQ_RELEASE set / unset; a pure function, the
 * rule rmx_step_seq's recording applies.
 * rmx_queue_counters: that queue's windows, kernel-argument uploads and packets so far for the handle's device.
 * rmx_queue_info: out[0..n) of RMX_QUEUE_INFO_N values: [0] windows, [1] uploads, [2] packets (as above), [3] windows
 * of the device served on a stream, [4] the device queue's state (RMX_QUEUE_*), [5] how the handle's last
 * rmx_step_seq ran (RMX_SEQ_*), [6] how often the handle re-recorded its window (a repeated identical call reuses
 * the recording and uploads nothing). */
int rmx_step_seq(rmx_handle* h, const int32_t* actions_dev, int64_t action_stride, int32_t n_steps, int autoreset,
                 double* stats_out_dev, void* hip_stream);
/* 1 if the handle's last rmx_step_seq ran on the queue as a packed window (the private layout above), else 0. */
int rmx_seq_packed(const rmx_handle* h);
int rmx_seq_handoff(int32_t k, int32_t n_steps, int packed, int release_all);
int rmx_queue_counters(const rmx_handle* h, int64_t* out3);
#define RMX_QUEUE_INFO_N 7
#define RMX_QUEUE_UNUSED 0      /* not set up yet (no window on this device so far) */
#define RMX_QUEUE_READY 1
#define RMX_QUEUE_UNAVAILABLE 2 /* set-up failed: windows run on the stream */
#define RMX_QUEUE_RETIRED 3     /* a window failed: later windows run on the stream */
#define RMX_SEQ_NONE 0            /* no rmx_step_seq on this handle yet */
#define RMX_SEQ_QUEUE 1           /* the engine's queue */
#define RMX_SEQ_STREAM_KERNEL 2   /* the stream: the handle's step is not the thread-per-env fast kernel */
#define RMX_SEQ_STREAM_DISABLED 3 /* the stream: RMX_QUEUE=0 at rmx_create */
#define RMX_SEQ_STREAM_QUEUE 4    /* the stream: the queue is unavailable or retired, or refused a kernel */
#define RMX_SEQ_HOST 5            /* a host handle: the K steps on the CPU */
int rmx_queue_info(const rmx_handle* h, int64_t* out, int32_t n);
/* Dispatch timing of the handle's device queue (profiling; off by default).  The queue has HSA dispatch profiling
 * enabled from its creation.  rmx_queue_timing(h, m), m >= 1: from the next window on, packets 0, m, 2m, ... and the
 * window's last one carry a completion signal of their own (at most 4,096 per window), so the command processor
 * stamps those dispatches' start (packet processing) and end (completion) — the timestamps a kernel trace reads, with
 * the packets still back to back behind one doorbell.  A stamped packet costs the command processor ~1.2 us more than
 * an unstamped one: m = 1 times every dispatch at that cost, a sparse m leaves the cadence as it is and the span
 * between stamps measures it.  m = 0 turns timing off.  rmx_queue_times: the last timed window's stamps into stamps
 * ([n][3]: packet index, start, end; ns in the system timestamp domain; at most cap triples) and *n their number (0:
 * no timed window yet, the last window was untimed or ran on the stream, or a host handle); they stay readable after
 * timing is turned off, until the next window.  Results are unchanged by timing. */
int rmx_queue_timing(rmx_handle* h, int every);
int rmx_queue_times(const rmx_handle* h, uint64_t* stamps, int64_t cap, int64_t* n);
/* The queue's metadata check (no GPU needed) over a gfx950 code object (co == NULL: the step code object embedded in
 * this library): *n_step_kernels step_fast_kernel instantiations found, *n_refused of them the queue would refuse;
 * the first refused one and why into report (NUL-terminated, truncated to report_cap).  -1 (RMX_E_INVALID) if the
 * object cannot be read. */
int rmx_code_object_check(const void* co, size_t bytes, int64_t* n_step_kernels, int64_t* n_refused, char* report,
                          size_t report_cap);

/* Which step kernel rmx_step / rmx_step_hashed launch for this handle (no device work):
 * RMX_VARIANT_GENERIC thread-per-env, RMX_VARIANT_LANE_PER_AGENT, or the deterministic fast path
 * (pre-composed move words; selected when the config allows it and no QRM outputs are bound) as
 * RMX_VARIANT_FAST (thread-per-env).  At rmx_create, RMX_FAST=0 in the environment disables the fast
 * path.  RMX_VARIANT_FAST_LANE_PER_AGENT is no longer returned (round 5 removed that layout after it lost
 * its A/Bs); the value stays reserved. */
#define RMX_VARIANT_GENERIC 0
#define RMX_VARIANT_LANE_PER_AGENT 1
#define RMX_VARIANT_FAST 2
#define RMX_VARIANT_FAST_LANE_PER_AGENT 3
#define RMX_VARIANT_HOST 4 /* a host handle (cfg.device == RMX_DEVICE_HOST): the CPU path */
int rmx_step_variant(const rmx_handle* h);

/* The kernel configuration rmx_create chose for this handle, after every fallback (no device work; no reference
 * counterpart): out[0..n) of RMX_STEP_INFO_N values.
 *   [0]  the step variant, as rmx_step_variant returns it
 *   [1]  the table mode the step kernel reads (RMX_TABLES_*): NONE for the generic kernels and host handles; GLOBAL
 *        also where QRM outputs are bound to a fast handle (the move word carries the event they need)
 *   [2]  bytes per merged record the step kernel reads: 16, 4 (RMX_TABLES_MERGED4), or 0 (no merged table read)
 *   [3]  agent sections stored in the merged table after identical ones are shared (0: no merged table)
 *   [4]  bytes of the 16-B merged records, [5] bytes of the 4-B records that follow them (0: none built)
 *   [6]  bytes of the fast path's blob (move words, RM entries; 0: the config is not eligible or RMX_FAST=0)
 *   [7]  bytes of the generic kernels' table blob (<= 64 KiB)
 *   [8]  the store mode of the step kernel in [0]: the fast kernel's (2 rm_q / ep_ret stores skipped when unchanged,
 *        3 the same with non-temporal stores) or the generic kernel's (0 every word stored, 1 unchanged words skipped)
 *   [9]  episode statistics: 1 per-wave slab, 0 per-env slots (fast kernel below 1M envs)
 *   [10] workgroup size of the step kernel
 *   [11] 1 if QRM outputs are bound and the fast kernel serves them
 *   [12] 1 if slip / random starts use the fixed-seed reset cache (seed_episode_stride == 0 on a fast handle)
 *   [13] the fused rollout's layout: 0 thread-per-env, 1 lane-per-agent
 * [0], [1], [2], [8], [10] and [11] depend on the bound buffers (QRM columns): ask after rmx_bind.
 * A host handle reports RMX_VARIANT_HOST and zeros. */
#define RMX_STEP_INFO_N 14
#define RMX_TABLES_NONE 0
#define RMX_TABLES_GLOBAL 1
#define RMX_TABLES_MERGED 2
#define RMX_TABLES_MERGED4 3
int rmx_step_info(const rmx_handle* h, int64_t* out, int32_t n);

/* ---- tabular Q-learning / QRM learners fused into the step ------------------------------------------------------
 * QLearning.update behind AgentRL.update_policy (learning_algorithms/qlearning.py:41-110, multi_agent/agent_rl.py:
 * 117-192) as the runners call it for every agent after every step (frozen_lake_main.py:345-376, office_main.py:
 * 1709-1749): one independent learner per (agent a, env e), i.e. N replicas of the runner's experiment.
 * Tables: caller-owned float64 q[A][N][S_max][4] and (optional) visits of the same shape, S_max = W*H*max_a enc_nq[a]
 * (rmx_learn_states); q[a][e] is that learner's q_table as the reference holds it ([state][action], state =
 * (y*W + x)*enc_nq[a] + rm index), rows past W*H*enc_nq[a] are never touched.  The caller fills q with qtable_init
 * and visits with 0; a device handle takes device pointers (16-byte aligned), a host handle host pointers.  Each table
 * is A * N * S_max * 4 doubles (N = cfg.n_envs): rmx_learn_bind cannot check the extent, and the learn step indexes
 * all of [A][N][S_max][4].
 * update_q (qlearning.py:70-79), each step one IEEE float64 operation, never fused:
 *   visits[s][k] += 1 (when bound); lr = learning_rate, or 1/visits[s][k] (correctly rounded) when learning_rate == 0
 *   (the reference's learning_rate=None; its constructor cannot be called with it, qlearning.py:37, its update can);
 *   maxq = 0 when done, else max(q[sn][0..3]);  a = (1-lr)*cur; b = gamma*maxq; c = r + b; d = lr*c; q[s][k] = a + d.
 * Experiences of one agent-step, strictly in order on the one table (a later one reads what an earlier one wrote):
 *   use_qrm: one update_q per RM state j of get_all_states()[:-1] (qlearning.py:82-106 over rm_environment_wrapper.py:
 *     140-183; the tuples of the qrm_* columns): s = prev_cell*nQ + q_j, sn = cell*nQ + nq_j, done = env_term ||
 *     nq_j == final, r = (double)Renv + (double)rq_j (the raw RM reward, rm_environment_wrapper.py:171), and with
 *     use_rsh r += gamma*phi[nq_j] - phi[q_j] in float64 (qlearning.py:93-105; gamma is the learner's);
 *   else one update_q: s = encode(pre-step position, pre-step RM state) (the reset state when the step auto-reset
 *     first), sn = encode(post-step ...), r = (double)Renv + (double)reward_modifier*(double)RQ, done = terminated ||
 *     (trunc_is_terminal && truncated): trunc_is_terminal = 1 is the FrozenLake runner (frozen_lake_main.py:359), 0 the
 *     OfficeWorld runner (office_main.py:1733).
 * Every agent updates every step, inactive and RM-final ones included, as the runners do.  An action without a table
 * column (RMX_WAIT, or an invalid one, reported as rmx_step reports it) is stepped and updates nothing.
 * use_rsh without use_qrm is refused: the reference's own non-QRM shaping looks a label-keyed dict up by RM index
 * (agent_rl.py:158-165, qlearning.py:60-66), which is not reproduced.
 * Dynamics (rmx_learn_config.dynamics): RMX_LEARN_DYN_FIXED (0, a zeroed config) serves deterministic dynamics and
 * fixed starts only: a config with cfg.stochastic or cfg.random_starts is refused.  RMX_LEARN_DYN_ENV follows the
 * handle: on a handle with cfg.stochastic and / or cfg.random_starts (office_main.py --stochastic, ma_frozen_lake.py:
 * 59-64 frozen_lake_stochastic / random_start_positions; rng and episode bound at rmx_bind as rmx_step needs them) the
 * learn step does, per env and in the order of the runner's loop:
 *   1. the auto-reset: for an env that resets, episode += 1, the env generator becomes default_rng(seed of that
 *      episode in the seed schedule), and the random starts are drawn from it, before any slip draw;
 *   2. the policy for every agent, frozen ones included, over the row of the state about to be left (the fresh,
 *      possibly random, start after a reset); it draws from the learner's own generator only;
 *   3. the step: the slip draws come from the env generator, in agent order, only for the agents that move;
 *   4. the update, with the INTENDED action (the policy's or the caller's, not the slipped one) and the state actually
 *      reached, as rm_environment_wrapper.py:140-183 and the runners hand them to update_policy.
 * The env generator (rng [4][N]) and the learner generators (rmx_learn_rng_bind) never mix: neither is drawn from
 * where the reference draws from the other.  On a deterministic handle RMX_LEARN_DYN_ENV runs the very kernels of
 * RMX_LEARN_DYN_FIXED.
 * Bit-exactness: q equals the reference's bit for bit whenever every reward, penalty and reward_modifier of the
 * scenario is a float32 value (the engine stores them as float32).
 * The engine's policy (rmx_learn_step_policy; its own, not numpy's stream; independent of the sharding), chosen after
 * the auto-reset from the row of the state the step is about to leave, for agent i of global env e at t_global:
 *   h0 = splitmix64(seed ^ (((t_global*N_global + e)*A + i) * 0x9E3779B97F4A7C15))  (rmx_fill_actions' value before
 *   its >> 62), h1 = splitmix64(h0), h2 = splitmix64(h1); explore iff (h1 >> 11) * 2^-53 < epsilon, with action
 *   h0 >> 62; else greedy: the row's maxima by float64 equality with the row maximum, in index order, maximum number
 *   ((h2 >> 32) * n_max) >> 32 (qlearning.py:137-143 with the engine's draw).  RMX_LEARN_BEST: the first maximum
 *   (np.argmax, qlearning.py:116-117).  The row maximum is m = row[0], then m = v for every later v > m: a NaN in
 *   row[0] stays, a NaN further on is skipped.  A row with no entry equal to its maximum (a NaN maximum) gives
 *   action 3, greedy and RMX_LEARN_BEST alike (the explore draw comes first and does not look at the row).
 *   A state outside the agent's W*H*enc_nq[a] rows (pos_x / pos_y / rm_q columns the caller overwrote out of range)
 *   reads a row of four zeros, never table memory; an experience whose s or sn is outside those rows is dropped:
 *   neither q nor visits is written (with use_rsh also when nq_j is no RM index, before phi is read).
 * The reference's policy (rmx_learn_step_policy with RMX_LEARN_NUMPY; seed and t_global are ignored): QLearning.
 * choose_action (qlearning.py:112-143, action_selection "greedy") on each learner's own np.random.default_rng(seed)
 * (learning_algorithm.py:32), as the runners call it through select_action for every agent every step, frozen and
 * inactive ones included (frozen_lake_main.py:269-295 seeds every learner with 2020, office_main.py:704-717 with
 * args.seed).  Learner (a, e) owns one PCG64 generator in the column bound by rmx_learn_rng_bind; on every such step
 * that is not RMX_LEARN_BEST, over the same row as above:
 *   d = (next_uint64() >> 11) * 2^-53 (Generator.uniform(0, 1)), drawn whatever epsilon is; explore iff d < epsilon,
 *   with action bounded(4); else greedy: m the row maximum by the rule above, k the number of entries equal to m, the
 *   action is maximum number bounded(k) in index order; k == 0 (a NaN maximum; the reference raises there) gives
 *   action 3 and draws nothing more.
 *   bounded(k) = Generator.choice of a k-sequence = integers(0, k), Lemire's method on buffered 32-bit draws: k == 1
 *   returns 0 and draws nothing; else m64 = (uint64)next_uint32() * k, left = (uint32)m64; if left < k then thr =
 *   (0xFFFFFFFF - (k-1)) % k and m64 is redrawn while left < thr; the result is m64 >> 32 (thr is 0 for k = 2 and 4:
 *   only k = 3 can redraw, on left == 0).  next_uint32() is PCG64's buffered draw: a buffered half is returned and
 *   the flag cleared, else 64 bits are drawn, the low half returned and the high half buffered; next_uint64() never
 *   touches the buffer.
 *   With RMX_LEARN_BEST as well, best wins: nothing is drawn and the column is not touched.  Without
 *   RMX_LEARN_UPDATE the draws still happen (select_action without update_policy).
 * Bit-exactness of a run: with epsilon as the reference's learner has it (both worlds' reset() call learn_done_episode
 * on every QLearning learner, ma_frozen_lake.py:86-88, ma_office.py:107-108; the runner scripts pin epsilon_start ==
 * epsilon_end, so there a fixed scalar epsilon serves; every other schedule: rmx_learn_eps_bind, "per-learner epsilon
 * schedules" below) and float32 rewards as above, the actions of every step, q, visits and each generator's state after T
 * steps equal those of the runner's loop (select_action for every agent, rm_env.step, update_policy for every agent)
 * bit for bit, on the device and on the host, whatever the sharding (a learner's stream depends on its own column
 * words only).  With RMX_LEARN_DYN_ENV this holds on slip and random-start worlds too, whose episodes the loop resets
 * with the seed schedule's seeds (rmx_reset, cfg.seed_*): the env columns, the env generator and the episode count then
 * equal the reference env's state, its rng.bit_generator.state and its number of resets as well (an env's stream
 * depends on the base seed, its global index and its episode only).
 * The generator column is caller-owned like q and visits: uint64 rng[5][A][N], plane-major, word w of learner (a, e)
 * at rng[(w*A + a)*N + e]: 0 state high, 1 state low, 2 increment high, 3 increment low (numpy's bit_generator.state
 * "state" / "inc" as 128-bit numbers), 4 (has_uint32 << 32) | uinteger.  A learn step reads a learner's five words
 * and writes words 0, 1 and, when it changed, 4.  A device handle takes a device pointer, a host handle a host
 * pointer, 16-byte aligned; NULL unbinds; the extent (5 * A * N words) cannot be checked; the column is not part of
 * rmx_get_state.  rmx_learn_rng_seed fills the bound column with default_rng(seeds[a][e]) (SeedSequence -> PCG64, any
 * uint64 seed; nothing buffered) from host seeds [A][N], in stream order, and returns when the column is written.
 * RMX_E_STATE: rmx_learn_rng_bind / rmx_learn_rng_seed before rmx_learn_bind, rmx_learn_rng_seed or RMX_LEARN_NUMPY
 * with no column bound; RMX_E_INVALID: a misaligned column, NULL seeds; each with a message, before any device work.
 * Each learn step is ONE launch on the caller's stream: auto-reset, action choice, step, update.  It leaves every
 * bound column (enc_state and the QRM columns included) and the episode statistics as rmx_step with the same actions
 * leaves them (the statistics through the generic kernels' per-wave slots: the integer ones equal, the return sum in
 * that kernel's association).  Without RMX_LEARN_UPDATE the step is an evaluation step: the tables are only read.
 * rmx_learn_bind copies phi (host [A][Q], Q = cfg.n_rm_states; required with use_rsh) and keeps q / visits
 * (visits: NULL unless learning_rate == 0 or the counts are wanted).  RMX_E_INVALID with a message, before any device
 * work: a NULL handle / config / q, gamma or learning_rate not finite or negative, no enc_nq, use_qrm with
 * n_qrm_max == 0, use_rsh without use_qrm or phi, 1/visits without visits, a dynamics value other than the two below,
 * cfg.stochastic / cfg.random_starts under RMX_LEARN_DYN_FIXED, epsilon outside [0, 1], unknown flags.  A learn step before rmx_bind or rmx_learn_bind: RMX_E_STATE.
 * Not served: rmx_step_seq windows (learn steps are stream launches; T of them in one launch: rmx_learn_run below,
 * rmx_learn_model_run for R-max and QR-max learners),
 * the dict API, the tables in rmx_get_state (they are the caller's).
 * Runs (rmx_learn_run): exactly T consecutive calls of rmx_learn_step_policy(h, epsilon, flags, seed, t_global + k,
 * autoreset = 1, actions_out ? actions_out + k*A*N : NULL, stream), k = 0..T-1, in ONE launch on a device handle
 * (one thread per env runs its T steps; state, t, the env generator and the episode count stay in registers and the
 * columns are stored once at the end).  The same three flags, whatever learner is bound (Q-learning or QRM, with or
 * without rsh and visits, Q(lambda) while rmx_learn_lambda_bind is active) and the learner's dynamics
 * (RMX_LEARN_DYN_ENV: slip, the per-episode reseed, random starts, the episode column).  Auto-reset is always on, as
 * in rmx_rollout; a run on the caller's own actions (rmx_learn_step's mode) is not served.  After the call everything
 * is as the T single steps leave it, bit for bit: every state column, the output columns (the LAST step's reward,
 * renv, shaping, env_done, enc_state and QRM columns), q and visits, the learners' generator column (words 0, 1 and
 * 4; the increment is never written), the env generator and episode columns, the trace lists and counts, and the
 * error word (the same RMX_E_TRACE when a bound cap overflows).  Episode statistics: the integer ones (episodes,
 * successes, sum of lengths) are equal; a device handle sums the returns per lane over the run and then per wave, so
 * the return sum is associated differently from T single steps and agrees to rounding (as rmx_rollout against
 * rmx_step).  A host handle runs the T steps one after the other: everything is equal there, the return sum too.
 * RMX_E_INVALID: T < 1 or T > RMX_LEARN_RUN_MAX (one launch stays bounded: at the slowest measured learn step 4096
 * steps are a few seconds), epsilon outside [0, 1], unknown flags.  RMX_E_STATE: before rmx_bind or rmx_learn_bind,
 * RMX_LEARN_NUMPY with no column bound.  Each with a message, before any device work.  Like every other entry point
 * the call ends a resident synchronous workgroup first. */
typedef struct rmx_learn_config {
  double gamma, learning_rate /* 0: 1/visits */;
  int32_t use_qrm, use_rsh, trunc_is_terminal, dynamics /* RMX_LEARN_DYN_* */;
  const double* phi; /* host [A][Q], required with use_rsh; copied */
} rmx_learn_config;
#define RMX_LEARN_DYN_FIXED 0 /* deterministic dynamics and fixed starts only (slip / random-start handles refused) */
#define RMX_LEARN_DYN_ENV 1   /* the handle's dynamics: slip, the per-episode reseed and random starts included */
#define RMX_LEARN_UPDATE 1
#define RMX_LEARN_BEST 2
#define RMX_LEARN_NUMPY 4 /* rmx_learn_step_policy: the reference's policy on the learners' own numpy generators */
int rmx_learn_states(const rmx_handle* h, int64_t* s_max);
int rmx_learn_bind(rmx_handle* h, const rmx_learn_config* cfg, double* q, double* visits);
/* rmx_step with the caller's actions, then the update */
int rmx_learn_step(rmx_handle* h, const int32_t* actions, int autoreset, void* hip_stream);
/* the policy's actions (written to actions_out [A][N] unless NULL), the step, and with RMX_LEARN_UPDATE the update */
int rmx_learn_step_policy(rmx_handle* h, double epsilon, int flags, uint64_t seed, int64_t t_global, int autoreset,
                          int32_t* actions_out, void* hip_stream);
/* T auto-reset policy steps (1 <= T <= RMX_LEARN_RUN_MAX) in one launch; actions_out [T][A][N] or NULL */
#define RMX_LEARN_RUN_MAX 4096
int rmx_learn_run(rmx_handle* h, int32_t T, double epsilon, int flags, uint64_t seed, int64_t t_global,
                  int32_t* actions_out /* [T][A][N] or NULL */, void* hip_stream);
/* the learners' numpy generators for RMX_LEARN_NUMPY: bind the caller's column [5][A][N] (NULL unbinds), seed it */
int rmx_learn_rng_bind(rmx_handle* h, uint64_t* rng);
int rmx_learn_rng_seed(rmx_handle* h, const uint64_t* seeds_host /* [A][N] */, void* hip_stream);

/* ---- Watkins Q(lambda) learners fused into the step ------------------------------------------------------------
 * QLearningLambda.update (learning_algorithms/qlearning_lambda.py:33-84) behind AgentRL.update_policy (multi_agent/
 * agent_rl.py:117-192), one learner per (agent a, env e) on the tables rmx_learn_bind bound (q filled with the
 * reference's zeros by the caller; visits optional unless learning_rate == 0).  rmx_learn_lambda_bind, after
 * rmx_learn_bind, turns the handle's learners into Q(lambda) ones: rmx_learn_step and rmx_learn_step_policy then run
 * the Q(lambda) learn step, still ONE launch, with the same three policies (choose_action is QLearning's, line for
 * line), the same dynamics (RMX_LEARN_DYN_ENV included) and the same columns and statistics.
 * The experience is the non-QRM one of the Q-learning section: s, sn, done (trunc_is_terminal as there) and
 * r = (double)Renv + (double)reward_modifier*(double)RQ; there is no QRM and no shaping (update ignores info), so a
 * learner bound with use_qrm or use_rsh is refused.  update_policy never passes next_action: update then takes the
 * argmax as the next action, which is always greedy, so under the reference's call path the traces always decay and
 * are never cut.  That path is what is reproduced; an explicit next_action is not served.
 * One update, i = s*4 + k, each step one IEEE float64 operation, never fused:
 *   visits[i] += 1; lr = learning_rate, or 1/visits[i] (correctly rounded) when learning_rate == 0;
 *   best = 0 when done, else max(q[sn][0..3]), read before any write of this update;
 *   td = (r + gamma*best) - q[i];  e[i] = 1 (replacing traces);  c = lr*td;  q[j] = q[j] + (c*e[j]) for every j;
 *   done: every trace of the learner becomes 0;  else g = gamma*lambd and e[j] = e[j]*g for every j.
 * The reference's e_table is dense and its update sweeps the whole table.  The engine keeps, per learner, the list
 * of its live traces, caller-owned like q and visits:
 *   trace_idx int32 [A][L][N], trace_val float64 [A][L][N], trace_cnt int32 [A][N] (the caller zeroes trace_cnt),
 *   slot-major: slot j of learner (a, e) at [(a*L + j)*N + e];  slots 0..cnt-1 hold distinct cells i, each with a
 *   trace that is not 0: a cell is listed iff its dense e would be non-zero.  A trace that decays to exactly 0
 *   (through the subnormals) leaves the list; order is kept.
 * Bit-exactness: adding c*0.0 leaves a float64 unchanged for every finite c and every value but -0.0 (-0.0 + 0.0 is
 * +0.0), so q, visits and the dense e rebuilt from the lists equal the reference's bit for bit, under the conditions
 * of the Q-learning section, for every initial q value but -0.0 (the reference starts at zeros) and while c stays
 * finite (an infinite or NaN c turns the reference's whole table to NaN).
 * Capacity: L = rmx_learn_lambda_slots() = 4*S_max can never overflow.  A caller may bind a smaller cap; under
 * auto-resetting learn steps a list never exceeds max_t + 1 entries.  A trace that finds its list full: the cell's own
 * update is applied, the trace is not kept, and the error word gets a bit that rmx_check_errors reports as
 * RMX_E_TRACE (an invalid action reported at the same time wins).  Nothing is ever written at or past slot cap.
 * When the lists are emptied: a learn step empties an env's lists when it auto-resets that env (env.reset() clears
 * every agent's traces whatever ended the episode, ma_frozen_lake.py:77-81, ma_office.py:100-102; an OfficeWorld
 * truncation passes terminated = False: the update decays, the reset wipes), before the policy reads its rows, with or
 * without RMX_LEARN_UPDATE; rmx_reset (the masked envs), rmx_reset_sync and rmx_set_state empty them on a handle with
 * Q(lambda) bound; rmx_learn_traces_clear(h, env_mask_dev, stream) empties those of the masked envs (NULL: all; a host
 * handle takes host bytes) in stream order.  rmx_step / rmx_step_hashed / rmx_step_report / rmx_step_seq /
 * rmx_rollout and the synchronous steps leave the lists alone, their auto-resets included: a caller who mixes them in
 * calls rmx_learn_traces_clear.  A step without RMX_LEARN_UPDATE touches no list but for the wipe above; nor does an
 * action without a table column, nor an experience whose s or sn is outside the agent's rows.
 * reset() does not call learn_done_episode on a QLearningLambda (it is no QLearning), so under the reference's
 * runners its epsilon stays fixed: leave the schedule unbound.  The class has a learn_done_episode of its own; a user
 * loop that calls it at every reset is what a bound schedule reproduces ("per-learner epsilon schedules" below).  Not
 * reproduced: an explicit next_action, softmax action selection.  The arrays are not part of rmx_get_state.
 * rmx_learn_lambda_bind: a NULL idx unbinds (Q-learning again); a later rmx_learn_bind drops the binding.  A device
 * handle takes device pointers, a host handle host pointers; the extents (A*cap*N, A*cap*N, A*N) cannot be checked.
 * RMX_E_INVALID with a message, before any device work: lambd not finite or outside [0, 1], cap < 1 or cap > 4*S_max,
 * a NULL val / cnt or an array not aligned to its element type (4, 8 and 4 bytes), a learner bound with use_qrm or
 * use_rsh.  RMX_E_STATE: before rmx_learn_bind (rmx_learn_traces_clear: before
 * rmx_learn_lambda_bind). */
int rmx_learn_lambda_slots(const rmx_handle* h, int32_t* l_full);
int rmx_learn_lambda_bind(rmx_handle* h, double lambd, int32_t cap, int32_t* trace_idx, double* trace_val,
                          int32_t* trace_cnt);
int rmx_learn_traces_clear(rmx_handle* h, const uint8_t* env_mask_dev, void* hip_stream);

/* ---- per-learner epsilon schedules: the reference's per-episode decay ---------------------------------------
 * QLearning owns its epsilon (qlearning.py:30-33; defaults epsilon_start = 1.0, epsilon_end = 0.2, epsilon_decay =
 * 0.99) and learn_done_episode (qlearning.py:153-155) sets epsilon = max(epsilon_end, epsilon * epsilon_decay).  Both
 * worlds' reset() call it on every QLearning learner at every reset (ma_frozen_lake.py:86-88, ma_office.py:107-108).
 * rmx_learn_eps_bind, after rmx_learn_bind, gives every learner its own epsilon: a caller-owned column like q, visits
 * and the generator column, float64 eps[A][N], learner (a, e) at eps[a*N + e], 8-byte aligned; a device handle takes a
 * device pointer, a host handle a host pointer; the caller fills it with epsilon_start, or with anything per learner
 * (an epsilon sweep across the replicas); NULL unbinds; the extent (A*N) cannot be checked; the column is not part of
 * rmx_get_state.  A later rmx_learn_bind drops the binding, as it drops the trace lists.
 * With a column bound, in rmx_learn_step_policy and rmx_learn_run learner (a, e) explores iff its draw is
 * < eps[a*N + e], under the engine's hashed policy and under RMX_LEARN_NUMPY alike (the draws themselves are as
 * without a column).  The scalar epsilon argument is validated as ever and otherwise ignored.  There is no flag bit:
 * the binding is state, as rmx_learn_lambda_bind's is.
 * Decay: an auto-reset of env e performed by a learn step (rmx_learn_step, rmx_learn_step_policy, every step of
 * rmx_learn_run) is the reference's env.reset(): each of the env's A learners gets x = eps*eps_decay (one IEEE float64
 * multiply), then eps = x > eps_end ? x : eps_end (Python's max(epsilon_end, x)), before the policy reads the column,
 * with or without RMX_LEARN_UPDATE, and under RMX_LEARN_BEST too (the reference's greedy episodes also go through
 * reset()).  autoreset = 0 resets nothing and decays nothing.  The result equals the reference's epsilon bit for bit.
 * Everything outside learn steps leaves the column alone, auto-resets included: rmx_reset, rmx_reset_sync,
 * rmx_set_state, rmx_step*, rmx_step_seq, rmx_rollout and the synchronous steps (unlike the trace lists, which the
 * resets empty).  How many resets precede the first step is the caller's business (the FrozenLake runner resets twice,
 * a plain loop once): rmx_learn_eps_decay(h, env_mask, stream) is learn_done_episode for every learner of the masked
 * envs (uint8 [N], NULL: all; a device handle takes a device mask, a host handle host bytes), in stream order.
 * Q(lambda) handles are served identically (see that section for what the reference does there).
 * Column values are not validated; the explore test is the plain float64 comparison draw < eps with draw in [0, 1):
 * a value > 1 always explores, a value <= 0 (and -0.0) never does, a NaN never does (every comparison with NaN is
 * false); a decay lifts every entry that is not above eps_end to eps_end, a NaN entry included (NaN > eps_end is
 * false), so such values last until the learner's env next resets.
 * RMX_E_STATE: either call before rmx_learn_bind, rmx_learn_eps_decay with no column bound.  RMX_E_INVALID: a NULL
 * handle, a misaligned column, eps_end outside [0, 1], eps_decay not finite or outside [0, 1].  Each with a message,
 * before any device work. */
int rmx_learn_eps_bind(rmx_handle* h, double* eps /* [A][N]; NULL unbinds */, double eps_end, double eps_decay);
int rmx_learn_eps_decay(rmx_handle* h, const uint8_t* env_mask /* NULL: all */, void* hip_stream);

/* ---- R-max learners: a learned model per learner, solved by value iteration ----------------------------------
 * RMax (learning_algorithms/rmax.py) behind AgentRL.update_policy, as the OfficeWorld runner builds it for
 * --algorithm RMAX / RMAXRM (office_main.py:663-684): one learner per (agent a, env e).  rmx_learn_bind comes first: q
 * is filled by the caller with max_reward/(1 - gamma), the visits table serves as s_a_counts and is required, use_rsh
 * is refused, learning_rate is unused.  rmx_learn_rmax_bind then turns the handle's learners into R-max ones;
 * rmx_learn_step and rmx_learn_step_policy run the R-max learn step (a device handle: at most two launches on the
 * caller's stream, rmx_learn_rmax.hip; no device synchronisation).  State encoding, the experiences of one agent-step
 * and the done rule (trunc_is_terminal) are those of the Q-learning section.
 * Caller-owned arrays beside q and visits, learner-major (a solve reads one learner's together):
 *   rsum float64 [A][N][S_max][4] (the reference's `rewards`), succ_idx / succ_cnt int32 [A][N][S_max][4][cap]: the
 *   non-zero entries of the reference's dense transitions[s][k][:] as a list, slot j of pair (s, k) of learner (a, e)
 *   at ((((a*N + e)*S_max + s)*4 + k)*cap + j; a slot with succ_cnt == 0 is empty; slots fill in first-seen order.
 *   The caller zeroes all three.
 * One update_q(s, k, r, sn, done), rmax.py:156-170, in this order:
 *   done: q[sn][0..3] = 0, the lists of (sn, 0..3) become the single entry (sn, threshold), counts[sn][0..3] =
 *         threshold; rsum[sn] is left alone; this triggers no solve;
 *   counts[s][k] < threshold: rsum[s][k] += r (one float64 add); counts[s][k] += 1; the count of successor sn in the
 *         list of (s, k) += 1 (appended with count 1 if new); if counts[s][k] == threshold now, the learned MDP is
 *         solved at once, before the next experience of the same step.
 * Experiences of one agent-step: the real one first (r = (double)Renv + (double)reward_modifier*(double)RQ, the
 * intended action), then with use_qrm every counterfactual in get_all_states()[:-1] order (r = (double)Renv +
 * (double)rq_j), the RM state actually held included once more: the reference double counts it, and so does the
 * engine.  An action without a table column, or an experience with s or sn outside the agent's rows, is dropped.
 * Value iteration (rmax.py:185-227) over mask = counts >= threshold, at most max_iter sweeps (the reference: 10000):
 *   v[n] = max(q[n][0..3]);  for every masked (s, k): new = rsum/counts + gamma * sum_slots (cnt_slot/counts)*v[idx],
 *   the sum in slot order from +0.0, each step one IEEE float64 operation, never fused;  the sweep has converged when
 *   |q - new| < vi_delta for every masked entry (vi_delta_rel: the difference divided by |q| where q != 0, taken as 0
 *   where q == 0), tested before anything is written;  otherwise q[mask] = new[mask], a Jacobi sweep.  Unmasked
 *   entries are never written by a solve.
 * Bit-exactness: the dense transitions row is non-zero exactly for the listed successors, and adding 0.0 changes no
 * float64 but -0.0, so the dense einsum over n is a sum of the listed terms; a sum of at most two of them does not
 * depend on the order, so on worlds where every (s, k) has at most two successors q equals the reference's bit for
 * bit, as counts, rsum and the lists always do.  With three or more successors numpy's einsum sums in another order:
 * q then agrees within 2*vi_delta/(1 - gamma) (both stop at a Bellman residual below vi_delta on the same model).
 * Policy (rmax.py:108-128): there is no epsilon; rmx_learn_step_policy validates its scalar and ignores it, and a
 * bound epsilon column is left alone (never read, never decayed).  A row whose four entries equal row[0] (float64
 * equality), unless RMX_LEARN_BEST: rng.choice of the four actions, which is integers(0, 4) on the learner's own
 * generator under RMX_LEARN_NUMPY (no other draw is made, and a row that is not flat draws nothing) and h0 >> 62 of
 * the engine's hashed policy otherwise.  Any other row, and every row under RMX_LEARN_BEST: the first maximum.  A
 * state outside the agent's rows reads as four zeros, which is therefore the random case.
 * Capacity: rmx_learn_rmax_slots() = 5 can never overflow.  The derivation, from agent_step (csrc/rmx_rules.h): the
 * cell after an agent-step is the agent's own or one of its four neighbours, whatever the slip outcome (a slip only
 * replaces the direction; a blocked move, a wall collision and a frozen agent stay put; a hole or a plant is entered
 * like any cell), so at most five cells; the next RM index is next_q[q][event(cell')] for the real experience and
 * for every counterfactual alike (a frozen agent's RM still steps on its own cell), a function of (q, cell'); other
 * agents never move or block an agent.  So sn is a function of (s, cell'), and (s, k) has at most five successors;
 * a deterministic world has one.  A caller may bind fewer.  A successor that finds its list full is still counted in
 * counts and rsum, its list entry is dropped, and the error word gets a bit that rmx_check_errors reports as
 * RMX_E_MODEL (an invalid action or a full trace list reported at the same time wins).  Nothing is written at or past
 * slot cap.
 * None of the arrays is part of rmx_get_state, and no reset touches them: env.reset() does nothing to an RMax.
 * rmx_learn_run on a handle with R-max bound: RMX_E_STATE (one thread per env cannot run a workgroup-wide solve);
 * rmx_learn_model_run below runs T steps of such a handle in one launch, one wave per env.  A device handle keeps the
 * values of the learner being solved in LDS, 16 B per state: S_max above 4064 is refused at bind (a host handle has no
 * such bound).
 * rmx_learn_rmax_bind: a NULL rsum unbinds (Q-learning steps on the same tables again); a later rmx_learn_bind drops
 * the binding; refused (RMX_E_STATE) while Q(lambda) lists are bound, as rmx_learn_lambda_bind is while a model is
 * bound, and before rmx_learn_bind.  RMX_E_INVALID with a message, before any device work: threshold < 1, vi_delta not
 * finite or <= 0, max_iter < 1, the learner's gamma >= 1, cap < 1 or above the full cap, a NULL or misaligned array
 * (8, 4 and 4 bytes), a learner bound with use_rsh or without visits.
 * rmx_learn_rmax_info: the solves made since the bind and the sweeps of the longest one (the converging sweep
 * included); it synchronises a device handle.
 * Not reproduced: noupdate_cnt and update's early-stop return value, QRMax_v2, UCBVI, OPSRL. */
int rmx_learn_rmax_slots(const rmx_handle* h, int32_t* cap_full);
int rmx_learn_rmax_bind(rmx_handle* h, int32_t threshold, double vi_delta, int vi_delta_rel, int32_t max_iter,
                        int32_t cap, double* rsum, int32_t* succ_idx, int32_t* succ_cnt);
int rmx_learn_rmax_info(rmx_handle* h, int64_t* solves, int64_t* max_sweeps);

/* ---- QR-max learners: a factored environment / RM model per learner, solved by value iteration -----------------
 * QRMax_v2 (learning_algorithms/qrmax_v2.py) behind AgentRL.update_policy, as the OfficeWorld runner builds it for
 * --algorithm QRMAX / QRMAXRM (create_qrmax, office_main.py:720-746): one learner per (agent a, env e).
 * rmx_learn_bind comes first: q is filled by the caller, per agent, with max_reward * enc_nq[a] / (1 - gamma) (R_max =
 * max_reward * nQ, qrmax_v2.py:38, 49); the visits table serves as nTSQA and is required; use_rsh is refused;
 * learning_rate is unused.  rmx_learn_qrmax_bind then turns the handle's learners into QR-max ones; rmx_learn_step and
 * rmx_learn_step_policy run the QR-max learn step (a device handle: at most two launches on the caller's stream,
 * rmx_learn_qrmax.hip; no device synchronisation).
 * Indices: s = y*W + x is the position (info["s"]), q the RM state index, P = W*H, nQ = enc_nq[a].  Q[s, q, a] is
 * q[(s*nQ + q)*4 + a] of the bound table.
 * Caller-owned arrays beside q and visits, learner-major, zeroed by the caller:
 *   known_tsqa uint8 [A][N][S_max][4]                      knownTSQA, the one known flag that needs stored state
 *   n_tsa, n_rsa int32, sum_rsa float64 [A][N][P][4]       nTSA, nRSA, sumRSA
 *   succ_idx, succ_cnt int32 [A][N][P][4][cap]             nTSAS_dict[(s, a)] in first-seen order with nTSAS; a slot
 *                                                          with succ_cnt == 0 is empty
 *   n_tqs, tq_next, n_rqs int32, sum_rqs float64 [A][N][S_max]   nTQS, the successor q' of (q, s'), nRQS, sumRQS,
 *                                                          all indexed by the encoded (s', q) = s'*nQ + q
 *   final uint8 [A][N][S_max]                              final_states as a mask over s*nQ + q
 * With thresholds >= 1 every known flag but knownTSQA equals count >= threshold between two experiences, so the
 * others are not stored: knownTSA = n_tsa >= nsamples_te, knownRSA = n_rsa >= nsamples_re, knownTQS = n_tqs >=
 * nsamples_tq, knownRQS = n_rqs >= nsamples_rq.
 * One update (qrmax_v2.py:414-506).  Experiences of one agent-step: the real one first (s, q, a, s1, q1, re = Renv, rq =
 * RQ = (double)reward_modifier*(double)rm_reward, the done rule of trunc_is_terminal), then with use_qrm every
 * counterfactual in get_all_states()[:-1] order (the same a and re, rq the raw RM reward, done = env_term or rm_done),
 * the RM state actually held included once more.  An action without a table column, or an experience with a
 * position or RM index outside the agent's own, is dropped.  Each experience, in this order:
 *   1. update_RSQA_RSA: done: final[s1*nQ + q1] = 1.  knownTSQA[s,q,a] == 0: visits[s,q,a] += 1.  knownTSA[s,a] == 0:
 *      the count of s1 in the list of (s, a) += 1 (appended with count 1 if new), n_tsa[s,a] += 1.  knownRSA[s,a] == 0:
 *      n_rsa[s,a] += 1, sum_rsa[s,a] += re (one float64 add).
 *   2. update_TQS_RQS: knownTQS[q,s1] == 0: n_tqs += 1, tq_next = q1.  knownRQS[q,s1] == 0: n_rqs += 1, sum_rqs += rq.
 *   3. check_known, in the reference's order: knownTSQA[s,q,a] is set if visits[s,q,a] >= nsamples_te, or by the
 *      shortcut: knownTSA[s,a] ALREADY set when this experience arrived and knownTQS[q,ss1], likewise as it stood
 *      when this experience arrived for ss1 == s1, for every listed successor ss1 of (s, a).  Then knownTSA,
 *      knownTQS[q,s1], knownRSA, knownRQS[q,s1] by their counts.
 * If any experience of the agent-step made something newly known, ONE solve_VI runs behind the last experience.
 * solve_VI (qrmax_v2.py:265-338): q[s,q,:] = 0 for every final (s, q) (here, not when the state was marked: the
 * policy sees the old row until the next solve).  delta = 1.0; while delta > vi_delta and fewer than max_iter sweeps
 * (the reference: 10000): a Jacobi sweep over every (s, q, a) with knownTSA && knownRSA && knownTSQA and (s, q) not
 * final:  rsa = sum_rsa/n_rsa;  for each listed s1 of (s, a) in list order with n_tqs[q,s1] > 0, q1 its successor:
 * tr = (n/n) * (cnt/n_tsa), the first factor 1.0 exactly; rqs = n_rqs > 0 ? sum_rqs/n_rqs : 0; qq1 += tr*(rsa + rqs);
 * qq2 += tr*max_a Q_old[s1,q1];  a successor whose (q, s1) was never observed contributes nothing;  Qnew = qq1 +
 * gamma*qq2;  cdelta = |Qnew - Qold|, under vi_delta_rel divided by m = |max(Qnew, Qold)| where m > 0;  delta is the
 * largest cdelta of the sweep (a NaN never raises it);  Q = Qnew after every sweep, the last one included.  Every
 * step is one IEEE float64 operation, never fused; the sums start from +0.0 in list order.  solve_VI is a scalar
 * loop over the learner's own lists, so every table equals the reference's bit for bit, on slip worlds too.
 * Policy (qrmax_v2.py:216-232): there is no epsilon (rmx_learn_step_policy validates its scalar and ignores it; a
 * bound epsilon column is left alone).  Under RMX_LEARN_NUMPY every call first shuffles the list of the four actions
 * on the learner's own generator (numpy's untyped Fisher-Yates: for i = 3, 2, 1 swap with random_interval(i) on
 * buffered 32-bit draws), under RMX_LEARN_BEST too; a flat row, unless RMX_LEARN_BEST, takes the shuffled list at
 * integers(0, 4); any other row its first maximum.  Under the engine's hashed policy a flat row takes h0 >> 62 and
 * nothing is drawn.  A state outside the agent's rows reads as four zeros, which is the flat case.
 * Capacity: rmx_learn_qrmax_slots() = 5 can never overflow: the position after an agent-step is the agent's own cell
 * or one of its four neighbours (the R-max derivation above, with positions in place of encoded states).  A caller
 * may bind fewer.  A successor that finds its list full is still counted in n_tsa, its entry is dropped, and the
 * error word gets the bit rmx_check_errors reports as RMX_E_MODEL.  Nothing is written at or past slot cap.
 * None of the arrays is part of rmx_get_state, and no reset touches them.  rmx_learn_run on a handle with QR-max
 * bound: RMX_E_STATE; rmx_learn_model_run below runs T steps of such a handle in one launch.  A device handle keeps
 * the values of the learner being solved in LDS, 16 B per state: S_max above 4064 is refused at bind (a host handle
 * has no such bound).
 * rmx_learn_qrmax_bind: a NULL known_tsqa unbinds (Q-learning steps on the same tables again); a later rmx_learn_bind
 * drops the binding; refused (RMX_E_STATE) while Q(lambda) lists or an R-max model are bound, as those binds are while
 * a QR-max model is bound, and before rmx_learn_bind.  RMX_E_INVALID with a message, before any device work: a
 * threshold < 1, vi_delta not finite or <= 0, max_iter < 1, the learner's gamma >= 1, cap < 1 or above the full cap, a
 * NULL or misaligned array, a learner bound with use_rsh or without visits.
 * rmx_learn_qrmax_info: the solves made since the bind, the sweeps of the longest one and the sweeps of all of them; it
 * synchronises a device handle.
 * Not reproduced: noupdate_cnt and update's early-stop return value; reset_VI; tosolve_VI / learn_done_episode (never
 * armed); save_environment / load_environment (the model arrays are the caller's: copy them); the bookkeeping no
 * computation reads (nTSQAS, nTSQA_dict, entrySQ_dict, nRSQA, nRSQASQ, sumR, pTSAS); UCBVI, OPSRL. */
int rmx_learn_qrmax_slots(const rmx_handle* h, int32_t* cap_full);
int rmx_learn_qrmax_bind(rmx_handle* h, int32_t nsamples_te, int32_t nsamples_re, int32_t nsamples_tq,
                         int32_t nsamples_rq, double vi_delta, int vi_delta_rel, int32_t max_iter, int32_t cap,
                         uint8_t* known_tsqa, int32_t* n_tsa, int32_t* n_rsa, double* sum_rsa, int32_t* succ_idx,
                         int32_t* succ_cnt, int32_t* n_tqs, int32_t* tq_next, int32_t* n_rqs, double* sum_rqs,
                         uint8_t* final);
int rmx_learn_qrmax_info(rmx_handle* h, int64_t* solves, int64_t* max_sweeps, int64_t* total_sweeps);

/* ---- runs of R-max and QR-max learners: T learn steps in one launch, one wave per env ----------------------------
 * rmx_learn_model_run on a handle with an R-max or a QR-max model bound: exactly T consecutive calls of
 * rmx_learn_step_policy(h, 0, flags, seed, t_global + k, autoreset = 1, actions_out ? actions_out + k*A*N : NULL,
 * stream), k = 0..T-1.  There is no epsilon (the model learners have none); the flags are rmx_learn_run's
 * (RMX_LEARN_UPDATE, RMX_LEARN_BEST, RMX_LEARN_NUMPY); auto-reset is always on; a run on the caller's own actions is
 * not served.
 * A device handle: ONE launch of one-wave workgroups, workgroup e owns env e (rmx_learn_rmax_run.hip,
 * rmx_learn_qrmax_run.hip).  Lane 0 of the wave is the one thread rmx_learn_run gives an env: state, t, the env
 * generator and the episode count stay in its registers over the T steps and the columns are stored once at the end;
 * it chooses the actions, steps the env and applies the model updates.  Every solve runs on all 64 lanes at the place
 * the reference has it: R-max at the crossing, before the next experience of the same agent-step (several crossings
 * in one agent-step: several solves); QR-max once behind the agent-step's last experience when anything became known.
 * No worklist, no record buffer and no second launch; envs never interact, so nothing synchronises across waves.
 * The staged tables and the solve's values (16 B per state) share the LDS of a plain launch, 64 KiB, 512 B of it
 * left to the kernel's own words.  Where the handle's table blob plus 16*S_max bytes exceed that, the call issues the
 * same T steps as T two-launch learn steps on the caller's stream instead: it never refuses a bound model.
 * After the call everything is as the T single steps leave it, bit for bit: every state column, the output columns
 * (the LAST step's), q, visits and every model array, the learners' generator column, the env generator and episode
 * columns, the solve statistics (rmx_learn_rmax_info / rmx_learn_qrmax_info) and the error word (the same
 * RMX_E_MODEL when a bound cap overflows).  Episode statistics: the integer ones are equal; a device handle sums the
 * returns per env over the run, so the return sum is associated differently from T single steps and agrees to
 * rounding.  A host handle runs the T steps one after the other: everything is equal there, the return sum too.
 * RMX_E_INVALID: a NULL handle, T < 1 or T > RMX_LEARN_MODEL_RUN_MAX, unknown flags.  RMX_E_STATE: before rmx_bind or
 * rmx_learn_bind; no model bound (rmx_learn_run is the entry for such handles); RMX_LEARN_NUMPY with no column bound.
 * Each with a message, before any device work.
 * RMX_LEARN_MODEL_RUN_MAX keeps one launch bounded, as RMX_LEARN_RUN_MAX does, but a model learner's worst step is
 * far slower than a Q-learning one: the slowest step measured is 11.4 ms (the first steps of a fresh R-max model at
 * threshold 1 with 65,536 envs, where almost every learner solves in every step).  256 such steps are about 3 s, and
 * still a few seconds if the fused kernel is twice as slow there. */
#define RMX_LEARN_MODEL_RUN_MAX 256
int rmx_learn_model_run(rmx_handle* h, int32_t T, int flags, uint64_t seed, int64_t t_global,
                        int32_t* actions_out /* [T][A][N] or NULL */, void* hip_stream);

/* Synchronise and report kernel-side errors (e.g. RMX_E_ACTION), then clear them. */
int rmx_check_errors(rmx_handle* h);

/* Checkpoint / resume of a rollout (the reference saves learner tables and pickles,
 * evaluation_metrics.py:193-214, office_main.py:1611-1613): everything needed to continue the bound shard
 * bit-exactly — the state columns pos_x, pos_y, rm_q, flags, ep_ret, t, the per-env rng / episode columns
 * when bound, the reset seed of the seed schedule and the episode statistics accumulated since the last
 * rmx_stats_clear — as ONE packed host blob of rmx_state_bytes() bytes (layout versioned by a header;
 * opaque to callers).  rmx_get_state synchronises the device and copies out; rmx_set_state checks the
 * header against the handle (A, N, rng columns; RMX_E_INVALID on mismatch), copies the columns into the
 * bound buffers and replaces the statistics, then synchronises. */
int rmx_state_bytes(const rmx_handle* h, size_t* bytes);
int rmx_get_state(rmx_handle* h, void* host_blob, size_t bytes);
int rmx_set_state(rmx_handle* h, const void* host_blob, size_t bytes);

/* ---- synchronous host-boundary calls: the reference's per-call dict API ---------------------------------
 * RMEnvironmentWrapper.reset(seed) / .step(actions) (rm_environment_wrapper.py:28-41, 43-107) as the reference
 * loops call them (frozen_lake_main.py:336-376, office_main.py:1696-1749): host actions in, host outputs back,
 * the call returns once they are there.  For small shards (n_envs <= RMX_SYNC_MAX_ENVS, typically 1).
 * One workgroup stays resident on the device between calls (state in registers, tables in LDS, a pinned
 * host mailbox polled by one lane): a call costs a host<->device round trip, not a kernel launch.  It exits
 * after RMX_SYNC_IDLE_US (default 2000) microseconds without a call, on rmx_sync_end, or implicitly at the
 * start of every other entry point on the handle, writing its state back to the bound device columns first.
 *   rmx_reset_sync: rmx_reset of every env with `seed` (the schedule's base seed), outputs after the reset;
 *   rmx_step_sync:  rmx_step with actions_host int32 [A][N] in host memory, outputs after the step;
 *                   RMX_E_ACTION (after stepping, the action treated as wait) for an action outside [0, 4] or
 *                   "wait" under FrozenLake slip (the reference raises KeyError);
 *   out_host:       host pointers laid out as the device columns of rmx_buffers (NULL fields are not copied;
 *                   rng / episode are ignored); shaping, enc_state and the QRM columns are available when the
 *                   handle computes them (cfg.has_shaping, cfg.enc_nq, QRM columns bound), else RMX_E_STATE;
 *   hip_stream:     the launch of the resident workgroup is ordered after the work enqueued on it so far.
 *   rmx_step_sync_begin + rmx_sync_wait: rmx_step_sync in two halves; the caller may do host work of its own
 *                   between them (no other call on the handle); rmx_sync_wait returns what rmx_step_sync would.
 * A request for N * A <= 15 actions travels inline in one 16-B request word (one host-memory read by the
 * device).  The resident workgroup runs on the handle's own non-blocking stream; a device-wide synchronisation
 * while it waits for a call returns when it times out. */
#define RMX_SYNC_MAX_ENVS 256
int rmx_reset_sync(rmx_handle* h, uint64_t seed, const rmx_buffers* out_host, void* hip_stream);
int rmx_step_sync(rmx_handle* h, const int32_t* actions_host, int autoreset, const rmx_buffers* out_host,
                  void* hip_stream);
int rmx_step_sync_begin(rmx_handle* h, const int32_t* actions_host, int autoreset, void* hip_stream);
int rmx_sync_wait(rmx_handle* h, const rmx_buffers* out_host);
int rmx_sync_end(rmx_handle* h);

#ifdef __cplusplus
}
#endif

#endif /* RMX_H */
