// rmx_capi_sync.cpp — the resident host-boundary stepper (rmx_sync.hip): the mailbox, rmx_reset_sync /
// rmx_step_sync* / rmx_sync_wait / rmx_sync_end.  Owns rmx_handle::sync.
#include <immintrin.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "rmx_handle.h"

using namespace rmx::capi;

namespace {

inline void cpu_relax() { __builtin_ia32_pause(); }

// Mailbox layout: request line | acknowledgement line | actions [A][N] | output columns in rmx_buffers order.
// The stream and the two events are created once per handle (rmx_bind frees only the mailbox, whose QRM sections
// follow the bound buffers); h->sync.mb is set last, so a failure part way leaves the next call to start over.
int sync_setup(rmx_handle* h) {
  if (h->sync.mb) return RMX_OK;
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  if (!h->sync.stream) HIP_TRY(hipStreamCreateWithFlags(&h->sync.stream, hipStreamNonBlocking), "resident stream");
  if (!h->sync.done) HIP_TRY(hipEventCreateWithFlags(&h->sync.done, hipEventDisableTiming), "resident event");
  if (!h->sync.dep) HIP_TRY(hipEventCreateWithFlags(&h->sync.dep, hipEventDisableTiming), "resident event");
  int khz = 0;
  HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device), "wall clock rate");
  const size_t A = (size_t)h->cfg.n_agents, N = (size_t)h->cfg.n_envs, AN = A * N;
  const size_t Qx = h->buf.qrm_s ? (size_t)h->cfg.n_qrm_max : 0;
  bool enc = true;
  for (int a = 0; a < h->cfg.n_agents; ++a) enc = enc && h->enc_nq[a] >= 1;
  size_t off = sizeof(rmx::SyncReq) + sizeof(rmx::SyncAck);
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off = (off + bytes + 15) & ~size_t(15);
    return o;
  };
  const size_t o_act = take(4 * AN), o_rec = take(32 * AN), o_env = take(16 * N);
  const size_t o_qs = Qx ? take(4 * AN * Qx) : 0, o_qsn = Qx ? take(4 * AN * Qx) : 0;
  const size_t o_qrq = Qx ? take(4 * AN * Qx) : 0, o_qd = Qx ? take(AN * Qx) : 0;
  h->sync.enc = enc;
  void* mb = nullptr;
  HIP_TRY(hipHostMalloc(&mb, off, hipHostMallocCoherent | hipHostMallocMapped), "mailbox hipHostMalloc");
  std::memset(mb, 0, off);
  void* dmb = nullptr;
  hipError_t e = hipHostGetDevicePointer(&dmb, mb, 0);
  if (e != hipSuccess) {
    (void)hipHostFree(mb);
    return hip_fail(e, "mailbox device pointer");
  }
  h->sync.bytes = off;
  unsigned char* d = static_cast<unsigned char*>(dmb);
  rmx::SyncIO& io = h->sync.io;
  io.req = reinterpret_cast<rmx::SyncReq*>(d);
  io.ack = reinterpret_cast<rmx::SyncAck*>(d + sizeof(rmx::SyncReq));
  io.act = reinterpret_cast<const int32_t*>(d + o_act);
  io.out = {reinterpret_cast<uint4*>(d + o_rec), reinterpret_cast<uint4*>(d + o_env),
            Qx ? reinterpret_cast<int32_t*>(d + o_qs) : nullptr, Qx ? reinterpret_cast<int32_t*>(d + o_qsn) : nullptr,
            Qx ? reinterpret_cast<float*>(d + o_qrq) : nullptr, Qx ? reinterpret_cast<uint8_t*>(d + o_qd) : nullptr};
  h->sync.mb = static_cast<unsigned char*>(mb);
  const double ticks_per_us = khz > 0 ? khz / 1000.0 : 100.0;
  double idle_us = 2000.0, life_ms = 10000.0;
  if (const char* v = std::getenv("RMX_SYNC_IDLE_US")) idle_us = std::max(0.0, std::atof(v));
  if (const char* v = std::getenv("RMX_SYNC_LIFE_MS")) life_ms = std::max(0.0, std::atof(v));
  if (const char* v = std::getenv("RMX_SYNC")) h->sync.oneshot = !std::strcmp(v, "launch") ? 1 : 0;
  h->sync.idle_ticks = (uint64_t)(idle_us * ticks_per_us);
  h->sync.life_ticks = h->sync.oneshot ? 0 : (uint64_t)(life_ms * 1000.0 * ticks_per_us);
  return RMX_OK;
}

// A host pointer into the mailbox for device pointer dp (the mailbox is mapped: same bytes, maybe another address).
template <typename T>
T* mb_host(const rmx_handle* h, T* dp) {
  const unsigned char* d0 = reinterpret_cast<const unsigned char*>(h->sync.io.req);
  return dp ? reinterpret_cast<T*>(h->sync.mb + (reinterpret_cast<const unsigned char*>(dp) - d0)) : nullptr;
}

int sync_launch(rmx_handle* h, void* stream) {
  // start after the work already enqueued on the caller's stream (e.g. the reset that wrote the columns)
  HIP_TRY(hipEventRecord(h->sync.dep, as_stream(stream)), "resident dependency");
  HIP_TRY(hipStreamWaitEvent(h->sync.stream, h->sync.dep, 0), "resident dependency");
  rmx::KParams p = base_params(h);
  rmx::SyncIO io = h->sync.io;
  io.seq0 = h->sync.served;
  io.idle_ticks = h->sync.idle_ticks;
  io.life_ticks = h->sync.life_ticks;
  HIP_TRY(rmx::launch_resident(p, io, h->cfg.kind, (int)h->cfg.n_envs, h->tables_bytes, h->sync.stream), "resident launch");
  HIP_TRY(hipEventRecord(h->sync.done, h->sync.stream), "resident event");
  h->sync.running = true;
  return RMX_OK;
}

// The request word {seq, ctl, acts, seq} goes out as ONE aligned 16-B store (x86: atomic for aligned 16-B
// vector stores), after everything it refers to (the action array, the seed): stores retire in order.
void sync_post(rmx_handle* h, uint32_t ctl, uint32_t acts) {
  rmx::SyncReq* r = mb_host(h, h->sync.io.req);
  const uint32_t seq = h->sync.seq + 1;
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  _mm_store_si128(reinterpret_cast<__m128i*>(r), _mm_set_epi32((int)seq, (int)acts, (int)ctl, (int)seq));
  h->sync.seq = seq;
}

// Post one request (launching the resident workgroup if none is running) without waiting for it.
int sync_begin(rmx_handle* h, uint32_t op, uint32_t autoreset, uint64_t seed, const int32_t* actions, void* stream) {
  uint32_t ctl = op | (autoreset ? rmx::kSyncAutoreset : 0u), acts = 0;
  if (op == rmx::kSyncReset) mb_host(h, h->sync.io.req)->seed = seed;
  if (actions) {
    const int64_t n = (int64_t)h->cfg.n_agents * h->cfg.n_envs;
    if (n <= rmx::kSyncInlineActs) {  // inline: 4-bit fields, k < 7 in ctl from bit 4, the rest in acts
      ctl |= rmx::kSyncInline;
      for (int64_t k = 0; k < n; ++k) {
        const uint32_t a = (uint32_t)actions[k] <= (uint32_t)RMX_WAIT ? (uint32_t)actions[k] : rmx::kSyncBadAct;
        if (k < 7)
          ctl |= a << (4 + 4 * k);
        else
          acts |= a << (4 * (k - 7));
      }
    } else {
      std::memcpy(const_cast<int32_t*>(mb_host(h, h->sync.io.act)), actions, sizeof(int32_t) * n);
    }
  }
  sync_post(h, ctl, acts);
#ifdef RMX_DIAG
  h->sync.t_post = std::chrono::steady_clock::now();
#endif
  h->sync.pending = true;
  h->sync.caller = stream;
  if (!h->sync.running) {
    HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
    return sync_launch(h, stream);
  }
  return RMX_OK;
}

// Wait for the posted request's acknowledgement.  A workgroup that timed out before it saw the request is
// relaunched with seq0 = the last served request, so the pending one is served exactly once.
int sync_wait(rmx_handle* h) {
  if (!h->sync.pending) return fail(RMX_E_STATE, "no synchronous request is outstanding");
  const rmx::SyncAck* ack = mb_host(h, h->sync.io.ack);
  const uint32_t seq = h->sync.seq;
  int rc;
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  for (unsigned spins = 1;; ++spins) {
    if (__atomic_load_n(&ack->seq, __ATOMIC_ACQUIRE) == seq) break;
    if ((spins & 63u) == 0) {
      const auto el = clk::now() - t0;
      if (el > std::chrono::microseconds(20)) {  // a normal round trip is a few us: has the workgroup exited?
        const hipError_t q = hipEventQuery(h->sync.done);
        if (q == hipSuccess) {
          if (__atomic_load_n(&ack->seq, __ATOMIC_ACQUIRE) == seq) break;
          h->sync.running = false;
          HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
          if ((rc = sync_launch(h, h->sync.caller))) return rc;
        } else if (q != hipErrorNotReady) {
          h->sync.running = false;
          h->sync.pending = false;
          return hip_fail(q, "resident stepper");
        }
        if (el > std::chrono::seconds(30)) return fail(RMX_E_HIP, "resident stepper did not acknowledge in 30 s");
      }
    }
    cpu_relax();
  }
#ifdef RMX_DIAG
  h->sync.wait_ns = std::chrono::duration<double, std::nano>(clk::now() - h->sync.t_post).count();
#endif
  h->sync.served = seq;
  h->sync.pending = false;
  if (h->sync.oneshot) {  // the workgroup exits by itself after one request: wait for it, relaunch on the next
    HIP_TRY(hipEventSynchronize(h->sync.done), "resident exit");
    h->sync.running = false;
  }
  return RMX_OK;
}

int sync_request(rmx_handle* h, uint32_t op, uint32_t autoreset, uint64_t seed, const int32_t* actions, void* stream) {
  const int rc = sync_begin(h, op, autoreset, seed, actions, stream);
  return rc ? rc : sync_wait(h);
}

// Unpack the columns the caller asked for from the mailbox's records; a requested column the handle does not
// compute fails.
int sync_copy_out(const rmx_handle* h, const rmx_buffers* out) {
  if (!out) return RMX_OK;
  const int64_t A = h->cfg.n_agents, N = h->cfg.n_envs;
  const size_t AQN = (size_t)(A * N) * (size_t)(h->buf.qrm_s ? h->cfg.n_qrm_max : 0);
  const rmx::SyncCols& c = h->sync.io.out;
  if (out->shaping && !h->cfg.has_shaping) return fail(RMX_E_STATE, "sync output column not computed: shaping");
  if (out->enc_state && !h->sync.enc) return fail(RMX_E_STATE, "sync output column not computed: enc_state");
  if ((out->qrm_s || out->qrm_sn || out->qrm_rq || out->qrm_done) && !c.qrm_s)
    return fail(RMX_E_STATE, "sync output columns not computed: QRM (bind the QRM columns)");
  const uint4* rec = mb_host(h, c.rec);
  const uint4* env = mb_host(h, c.envrec);
  auto f32 = [](uint32_t v) {
    float f;
    std::memcpy(&f, &v, 4);
    return f;
  };
  for (int64_t e = 0; e < N; ++e) {
    if (out->t) out->t[e] = (int32_t)env[e].x;
    if (out->env_done) out->env_done[e] = (uint8_t)env[e].y;
    for (int64_t a = 0; a < A; ++a) {
      const uint4 w0 = rec[2 * (e * A + a)], w1 = rec[2 * (e * A + a) + 1];
      const int64_t k = a * N + e;
      if (out->pos_x) out->pos_x[k] = (int32_t)(w0.x & 0xFFFFu);
      if (out->pos_y) out->pos_y[k] = (int32_t)(w0.x >> 16);
      if (out->rm_q) out->rm_q[k] = (int32_t)w0.y;
      if (out->flags) out->flags[k] = w0.z;
      if (out->reward) out->reward[k] = f32(w0.w);
      if (out->renv) out->renv[k] = f32(w1.x);
      if (out->ep_ret) out->ep_ret[k] = f32(w1.y);
      if (out->shaping) out->shaping[k] = f32(w1.z);
      if (out->enc_state) out->enc_state[k] = (int32_t)w1.w;
    }
  }
  if (out->qrm_s) std::memcpy(out->qrm_s, mb_host(h, c.qrm_s), 4 * AQN);
  if (out->qrm_sn) std::memcpy(out->qrm_sn, mb_host(h, c.qrm_sn), 4 * AQN);
  if (out->qrm_rq) std::memcpy(out->qrm_rq, mb_host(h, c.qrm_rq), 4 * AQN);
  if (out->qrm_done) std::memcpy(out->qrm_done, mb_host(h, c.qrm_done), AQN);
  return RMX_OK;
}

int sync_check(rmx_handle* h) {
  int rc = check_bound(h);
  if (rc) return rc;
  if (h->cfg.n_envs > RMX_SYNC_MAX_ENVS)
    return fail(RMX_E_INVALID, "rmx_*_sync serve shards of at most RMX_SYNC_MAX_ENVS envs");
  return sync_setup(h);
}

// The synchronous calls on a host handle: the step runs in rmx_step_sync_begin, rmx_sync_wait returns its outputs.
int host_sync_out(rmx_handle* h, const rmx_buffers* out, uint32_t bad) {
  if (out) {
    const std::string msg = h->host->copy_out(*out);
    if (!msg.empty()) return fail(RMX_E_STATE, msg);
  }
  if (bad) return fail(RMX_E_ACTION, "an action outside [0,4] (or wait under FrozenLake slip) was stepped (treated as wait)");
  return RMX_OK;
}

}  // namespace

int rmx::capi::sync_end(rmx_handle* h) {
  if (h && h->sync.pending) {  // a begun request is served first
    const int rc = sync_wait(h);
    if (rc) return rc;
  }
  if (!h || !h->sync.running) return RMX_OK;
  sync_post(h, rmx::kSyncExit, 0);
  h->sync.running = false;
  h->sync.served = h->sync.seq;  // nobody serves an exit request; later launches skip it
  HIP_TRY(hipEventSynchronize(h->sync.done), "resident exit");
  return RMX_OK;
}

extern "C" {

int rmx_reset_sync(rmx_handle* h, uint64_t seed, const rmx_buffers* out_host, void* stream) {
  if (h && h->host) {  // reset every env, then the columns after it (no step outputs: zeros)
    int rc = check_bound(h);
    if (rc) return rc;
    h->host->pending = false;
    h->host->reset(nullptr, seed);
    h->base_seed = seed;
    h->host->last_reset = true;
    return host_sync_out(h, out_host, 0);
  }
  int rc = sync_check(h);
  if (rc) return rc;
  if (h->sync.pending && (rc = sync_wait(h))) return rc;
  h->base_seed = seed;
  h->rs_dirty = false;  // the resident kernel resets every env from the new seed
  // the start cache / precompute tags follow on the stream of the next fast launch (starts_current): a memset here
  // on the caller's stream would not be ordered before a launch on another stream
  h->rs_stale = h->d_rsc || h->d_nx;
  if ((rc = sync_request(h, rmx::kSyncReset, 0, seed, nullptr, stream))) return rc;
  if ((rc = lambda_clear(h, nullptr, stream))) return rc;  // env.reset() clears every learner's traces
  return sync_copy_out(h, out_host);
}

int rmx_step_sync_begin(rmx_handle* h, const int32_t* actions_host, int autoreset, void* stream) {
  if (h && h->host) {  // the step itself; rmx_sync_wait returns its outputs
    int rc = check_bound(h);
    if (rc) return rc;
    if (!actions_host) return fail(RMX_E_INVALID, "actions is NULL");
    if (h->host->pending) return fail(RMX_E_STATE, "a synchronous request is outstanding (rmx_sync_wait first)");
    h->host->pending_bad = h->host->step(actions_host, autoreset);
    h->host->pending = true;
    h->host->last_reset = false;
    return RMX_OK;
  }
  int rc = sync_check(h);
  if (rc) return rc;
  if (!actions_host) return fail(RMX_E_INVALID, "actions is NULL");
  if (h->sync.pending) return fail(RMX_E_STATE, "a synchronous request is outstanding (rmx_sync_wait first)");
  return sync_begin(h, rmx::kSyncStep, autoreset ? 1u : 0u, 0, actions_host, stream);
}

int rmx_sync_wait(rmx_handle* h, const rmx_buffers* out_host) {
  if (!h) return fail(RMX_E_INVALID, "handle is NULL");
  if (h->host) {
    if (!h->host->pending) return fail(RMX_E_STATE, "no synchronous request is outstanding");
    h->host->pending = false;
    return host_sync_out(h, out_host, h->host->pending_bad);
  }
  int rc = sync_wait(h);
  if (rc) return rc;
  if ((rc = sync_copy_out(h, out_host))) return rc;
  if (__atomic_load_n(&mb_host(h, h->sync.io.ack)->bad, __ATOMIC_RELAXED))
    return fail(RMX_E_ACTION, "an action outside [0,4] (or wait under FrozenLake slip) was stepped (treated as wait)");
  return RMX_OK;
}

int rmx_step_sync(rmx_handle* h, const int32_t* actions_host, int autoreset, const rmx_buffers* out_host,
                  void* stream) {
  const int rc = rmx_step_sync_begin(h, actions_host, autoreset, stream);
  return rc ? rc : rmx_sync_wait(h, out_host);
}

int rmx_sync_end(rmx_handle* h) {
  if (!h) return fail(RMX_E_INVALID, "handle is NULL");
  if (h->host) {  // a begun request's outputs are dropped; the columns are current
    h->host->pending = false;
    return RMX_OK;
  }
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  return sync_end(h);
}

#ifdef RMX_DIAG
// Diagnostic builds only (not part of include/rmx.h): the resident stepper's device-side span of the last
// request (wall-clock ticks from seeing the request to its outputs being complete) and the tick rate in kHz.
int rmx_diag_sync_span(rmx_handle* h, unsigned long long* out /* [4]: t_seen, t_done, tick kHz, host post->ack ns */) {
  if (!h || !h->sync.mb) return fail(RMX_E_STATE, "no synchronous call made");
  const rmx::SyncAck* a = mb_host(h, h->sync.io.ack);
  int khz = 0;
  HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device), "wall clock rate");
  out[0] = a->t_seen;
  out[1] = a->t_done;
  out[2] = (unsigned long long)khz;
  out[3] = (unsigned long long)h->sync.wait_ns;
  return RMX_OK;
}
#endif

}  // extern "C"
