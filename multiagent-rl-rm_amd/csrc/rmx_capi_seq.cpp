// rmx_capi_seq.cpp — rmx_step_seq (window recording and reuse, packed-window eligibility) and the queue-info
// entry points.  Owns rmx_handle::seq.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <exception>

#include "rmx_handle.h"

using namespace rmx::capi;

// Packed windows serve the handles whose step is the default deterministic one: the merged-table step_fast_kernel with
// caller actions, the kSkipRare store set and per-env statistics slots (below 1M envs), no QRM outputs, no slip, fixed
// starts.  Everything else (and RMX_SEQ_PACKED=0, and a handle whose record buffer could not be allocated) keeps the
// window of K column-to-column steps.
static bool seq_packs(const rmx_handle* h) {
  const int tm = h->fast_tables;
  // (below 1M envs also keeps the record's byte offsets, (3A + 1) * N * 4, far inside the buffer descriptor's 32 bits)
  return !h->seq.packed_off && !h->seq.pk_failed && !h->seq.pk_refused && h->cfg.n_envs < kFastWaveStatsMinEnvs &&
         rmx::pk_bytes(h->cfg.n_agents, (size_t)h->cfg.n_envs) < ((size_t)1 << 31) && fast_applies(h) && !h->cfg.stochastic && !h->cfg.random_starts &&
         !h->buf.qrm_s && !h->fast_wave_stats && h->fast_skip == rmx::kSkipRare &&
         (tm == rmx::kTblMerged4 || tm == rmx::kTblMerged) && h->cfg.n_agents <= rmx::kFastMaxAgents;
}

// The record buffer of a handle's packed windows, allocated by its first one; false (remembered) when it cannot be
static bool seq_pack_buffer(rmx_handle* h) {
  if (h->seq.d_pk) return true;
  if (hipMalloc(&h->seq.d_pk, rmx::pk_bytes(h->cfg.n_agents, (size_t)h->cfg.n_envs)) != hipSuccess) {
    (void)hipGetLastError();  // not an error of the call: the window runs unpacked
    h->seq.d_pk = nullptr;
    h->seq.pk_failed = true;
    return false;
  }
  return true;
}

// The K launches rmx_step / rmx_step_report would issue, recorded (rmx::tl_capture) instead; false when the handle's
// step is not the thread-per-env step_fast_kernel.  packed (K >= 2): the same K packets as step_fast_kernel_win's I/O
// modes, the first one reading the columns, the last one writing them, the ones between on the handle's records.
static bool record_seq(rmx_handle* h, const int32_t* actions, int64_t stride, int32_t K, int autoreset,
                       double* stats_out, bool fused, bool packed) {
  h->seq.window.resize((size_t)K);
  for (int32_t k = 0; k < K; ++k) {
    const int32_t* a = actions + (size_t)k * (size_t)stride;
    const bool rpt = fused && k == K - 1;
    rmx::FastParams fp = rpt ? report_fp(h, a, autoreset, stats_out) : step_fp(h, a, 0, 0, autoreset);
    if (packed) fp.pk_io = k == 0 ? rmx::kIoColsToPk : (k == K - 1 ? rmx::kIoPkToCols : rmx::kIoPkToPk);
    rmx::StepCapture cap{&h->seq.window[(size_t)k], false};
    rmx::tl_capture = &cap;
    (void)rmx::launch_step_fast(fp, 0, h->cfg.kind, nullptr);
    rmx::tl_capture = nullptr;
    if (!cap.ok) return false;
    // the kernel side's dispatch must have taken the window kernel: a mixed window would read columns nobody wrote
    if (packed && !std::strstr(h->seq.window[(size_t)k].symbol, "step_fast_kernel_win")) return false;
    // packets 0 .. K - 2 of a packed window leave only the handle's record and statistics slots behind, all written
    // through: no release fence (queue_run); the last packet, which writes the caller's columns, keeps both fences
    h->seq.window[(size_t)k].handoff = rmx::seq_handoff(k, K, packed, h->seq.release_all) ? 1u : 0u;
  }
  return true;
}

static std::atomic<uint64_t> g_seq_keys{0};
// a window's recorded launches take ~1.2 KB of host memory and ~1.3 KB of kernel arguments each
constexpr int32_t kSeqMaxSteps = 1 << 20;

static int step_seq(rmx_handle* h, const int32_t* actions_dev, int64_t action_stride, int32_t n_steps, int autoreset,
                    double* stats_out_dev, void* stream) {
  int rc = check_bound(h);
  if (rc) return rc;
  if (!actions_dev || n_steps <= 0 || action_stride < 0) return fail(RMX_E_INVALID, "bad rmx_step_seq arguments");
  if (h->host) {  // the K steps in order on the host
    h->seq.dispatch = RMX_SEQ_HOST;
    for (int32_t k = 0; k < n_steps; ++k) h->host->step(actions_dev + (size_t)k * (size_t)action_stride, autoreset);
    if (stats_out_dev) std::memcpy(stats_out_dev, h->host->stats, sizeof(h->host->stats));
    return RMX_OK;
  }
  SYNC_END_OR_RETURN(h);
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  if ((rc = starts_current(h, stream))) return rc;
  hipStream_t st = as_stream(stream);
  const bool fused = stats_out_dev && report_fuses(h);
  // the K calls on the caller's stream, then a synchronisation: handles whose step is not the thread-per-env fast
  // kernel, RMX_QUEUE=0, and windows the queue cannot serve
  auto on_stream = [&](int why) {
    h->seq.dispatch = why;
    for (int32_t k = 0; k < n_steps; ++k) {
      const int32_t* a = actions_dev + (size_t)k * (size_t)action_stride;
      const int r = stats_out_dev && k == n_steps - 1 ? rmx_step_report(h, a, autoreset, stats_out_dev, stream)
                                                      : do_step(h, a, 0, 0, 0, autoreset, stream);
      if (r) return r;
    }
    HIP_TRY(hipStreamSynchronize(st), "step sequence");
    return (int)RMX_OK;
  };
  if (!fast_applies(h) || h->seq.queue_off) {
    rmx::queue_note_stream(h->device);
    return on_stream(h->seq.queue_off && fast_applies(h) ? RMX_SEQ_STREAM_DISABLED : RMX_SEQ_STREAM_KERNEL);
  }
  // the window recorded by the previous call is this one when the parameter block and the arguments agree
  // (fast_params zero-fills the block and FastParams has no padding, rmx_internal.h: a byte compare is a field one)
  const bool packed = n_steps >= 2 && seq_packs(h) && seq_pack_buffer(h);
  rmx::FastParams base = fast_params(h);  // (with the record buffer, once there is one)
  const bool same = h->seq.key && h->seq.actions == actions_dev && h->seq.stride == action_stride &&
                    h->seq.k == n_steps && h->seq.autoreset == (autoreset ? 1 : 0) && h->seq.out == stats_out_dev &&
                    std::memcmp(&base, &h->seq.base, sizeof(base)) == 0;
  if (!same) {
    h->seq.key = 0;
    h->seq.is_packed = packed && record_seq(h, actions_dev, action_stride, n_steps, autoreset, stats_out_dev, fused, true);
    if (packed && !h->seq.is_packed) {  // this handle's dispatch goes elsewhere: no record buffer, no second try
      h->seq.pk_refused = true;
      (void)hipFree(h->seq.d_pk);
      h->seq.d_pk = nullptr;
      base = fast_params(h);
    }
    if (!h->seq.is_packed &&
        !record_seq(h, actions_dev, action_stride, n_steps, autoreset, stats_out_dev, fused, false)) {
      rmx::queue_note_stream(h->device);
      return on_stream(RMX_SEQ_STREAM_KERNEL);
    }
    ++h->seq.recordings;
    std::memcpy(&h->seq.base, &base, sizeof(base));
    h->seq.actions = actions_dev;
    h->seq.out = stats_out_dev;
    h->seq.stride = action_stride;
    h->seq.k = n_steps;
    h->seq.autoreset = autoreset ? 1 : 0;
    h->seq.key = ++g_seq_keys;
  }
  // the caller's work on the stream (and a start-cache refresh) before the window
  const hipError_t q = hipStreamQuery(st);
  if (q == hipErrorNotReady) HIP_TRY(hipStreamSynchronize(st), "step sequence");
  else if (q != hipSuccess) return hip_fail(q, "step sequence");
  std::string err;
  const int qr = rmx::queue_run(h->device, h->seq.window.data(), n_steps, h->seq.key, &err);
  if (qr == rmx::kQueueStream) return on_stream(RMX_SEQ_STREAM_QUEUE);  // nothing was submitted
  if (qr) {
    h->seq.key = 0;
    h->seq.dispatch = RMX_SEQ_QUEUE;
    return fail(RMX_E_HIP, err);
  }
  h->seq.dispatch = RMX_SEQ_QUEUE;
  if (stats_out_dev && !fused) {  // the report's second launch (the statistics reduction) on the stream
    HIP_TRY(reduce_stats(h, stats_out_dev, st), "stats launch");
    HIP_TRY(hipStreamSynchronize(st), "step sequence");
  }
  return RMX_OK;
}

extern "C" {

int rmx_step_seq(rmx_handle* h, const int32_t* actions_dev, int64_t action_stride, int32_t n_steps, int autoreset,
                 double* stats_out_dev, void* stream) {
  if (n_steps > kSeqMaxSteps) return fail(RMX_E_INVALID, "rmx_step_seq: more steps than one window takes");
  try {  // nothing may unwind through the C ABI (the recorded window and the queue's buffers allocate)
    return step_seq(h, actions_dev, action_stride, n_steps, autoreset, stats_out_dev, stream);
  } catch (const std::exception& e) {
    if (h) h->seq.key = 0;
    return fail(RMX_E_HIP, std::string("rmx_step_seq: ") + e.what());
  }
}

int rmx_seq_packed(const rmx_handle* h) {
  return h && !h->host && h->seq.dispatch == RMX_SEQ_QUEUE && h->seq.key && h->seq.is_packed ? 1 : 0;
}

int rmx_seq_handoff(int32_t k, int32_t n_steps, int packed, int release_all) {
  return rmx::seq_handoff(k, n_steps, packed != 0, release_all != 0) ? 1 : 0;
}

int rmx_queue_counters(const rmx_handle* h, int64_t* out3) {
  if (!h || !out3) return fail(RMX_E_INVALID, "bad rmx_queue_counters arguments");
  rmx::QueueInfo qi{0, 0, 0, 0, RMX_QUEUE_UNUSED};  // a host handle has no device queue
  if (!h->host) rmx::queue_info(h->device, &qi);
  out3[0] = qi.windows;
  out3[1] = qi.uploads;
  out3[2] = qi.packets;
  return RMX_OK;
}

int rmx_queue_info(const rmx_handle* h, int64_t* out, int32_t n) {
  if (!h || !out || n < 0) return fail(RMX_E_INVALID, "bad rmx_queue_info arguments");
  rmx::QueueInfo qi{0, 0, 0, 0, RMX_QUEUE_UNUSED};  // a host handle has no device queue
  if (!h->host) rmx::queue_info(h->device, &qi);
  const int64_t v[RMX_QUEUE_INFO_N] = {qi.windows,         qi.uploads,      qi.packets, qi.stream_windows, qi.state,
                                       h->seq.dispatch, h->seq.recordings};
  for (int32_t i = 0; i < n && i < RMX_QUEUE_INFO_N; ++i) out[i] = v[i];
  return RMX_OK;
}

int rmx_queue_timing(rmx_handle* h, int every) {
  if (!h || every < 0) return fail(RMX_E_INVALID, "bad rmx_queue_timing arguments");
  if (h->host) return RMX_OK;  // a host handle has no device queue: nothing to time
  rmx::queue_set_timing(h->device, every);
  return RMX_OK;
}

int rmx_queue_times(const rmx_handle* h, uint64_t* stamps, int64_t cap, int64_t* n) {
  if (!h || !n || cap < 0 || (cap > 0 && !stamps)) return fail(RMX_E_INVALID, "bad rmx_queue_times arguments");
  // the device's last timed window, if this handle's last window ran on the queue
  *n = h->host || h->seq.dispatch != RMX_SEQ_QUEUE ? 0 : rmx::queue_times(h->device, stamps, cap);
  return RMX_OK;
}

int rmx_code_object_check(const void* co, size_t bytes, int64_t* n_step_kernels, int64_t* n_refused, char* report,
                          size_t report_cap) {
  if (!n_step_kernels || !n_refused || (co && bytes == 0)) return fail(RMX_E_INVALID, "bad rmx_code_object_check arguments");
  try {
    std::string first;
    const int rc = rmx::code_object_check(co, bytes, n_step_kernels, n_refused, &first);
    if (report && report_cap) {
      const size_t n = std::min(first.size(), report_cap - 1);
      std::memcpy(report, first.data(), n);
      report[n] = 0;
    }
    return rc ? fail(RMX_E_INVALID, "rmx_code_object_check: " + first) : RMX_OK;
  } catch (const std::exception& e) {
    return fail(RMX_E_INVALID, std::string("rmx_code_object_check: ") + e.what());
  }
}

}  // extern "C"
