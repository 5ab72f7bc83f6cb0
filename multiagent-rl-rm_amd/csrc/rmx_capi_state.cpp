// rmx_capi_state.cpp — the checkpoint blob: rmx_state_bytes / rmx_get_state / rmx_set_state.
#include <cstring>
#include <vector>

#include "rmx_handle.h"

using namespace rmx::capi;

namespace {

// rmx_get_state / rmx_set_state blob: header, then the columns in this order (agent-major [A][N] each):
// pos_x i32, pos_y i32, rm_q i32, flags u32, ep_ret f32, t i32 [N], and when the rng columns are bound
// rng u64 [4][N], episode i32 [N].
struct StateHeader {
  char magic[8];  // "RMXSTATE"
  uint32_t version, has_rng;
  int64_t n_agents, n_envs;
  uint64_t base_seed;
  double stats[RMX_NSTATS];
  uint64_t digest;  // config_digest of the handle that wrote the blob (version 2)
  int64_t env_offset, n_envs_global;
};
constexpr uint32_t kStateVersion = 2;

struct StateCol {
  void* dev;
  size_t bytes;
};

int state_columns(const rmx_handle* h, std::vector<StateCol>& cols, bool& has_rng) {
  const size_t AN = (size_t)h->cfg.n_agents * h->cfg.n_envs, N = (size_t)h->cfg.n_envs;
  const rmx_buffers& b = h->buf;
  has_rng = b.rng != nullptr && b.episode != nullptr;
  cols = {{b.pos_x, 4 * AN}, {b.pos_y, 4 * AN}, {b.rm_q, 4 * AN}, {b.flags, 4 * AN}, {b.ep_ret, 4 * AN}, {b.t, 4 * N}};
  if (has_rng) {
    cols.push_back({b.rng, 32 * N});
    cols.push_back({b.episode, 4 * N});
  }
  return RMX_OK;
}

size_t state_blob_bytes(const std::vector<StateCol>& cols) {
  size_t n = sizeof(StateHeader);
  for (const auto& c : cols) n += c.bytes;
  return n;
}

}  // namespace

extern "C" {

int rmx_state_bytes(const rmx_handle* h, size_t* bytes) {
  int rc = check_bound(h);
  if (rc) return rc;
  if (!bytes) return fail(RMX_E_INVALID, "bytes is NULL");
  std::vector<StateCol> cols;
  bool has_rng = false;
  state_columns(h, cols, has_rng);
  *bytes = state_blob_bytes(cols);
  return RMX_OK;
}

int rmx_get_state(rmx_handle* h, void* host_blob, size_t bytes) {
  int rc = check_bound(h);
  if (rc) return rc;
  std::vector<StateCol> cols;
  bool has_rng = false;
  state_columns(h, cols, has_rng);
  if (!host_blob || bytes != state_blob_bytes(cols)) return fail(RMX_E_INVALID, "state blob NULL or of the wrong size");
  if (!h->host) {
    SYNC_END_OR_RETURN(h);
    HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
    HIP_TRY(hipDeviceSynchronize(), "sync before get_state");
  }
  StateHeader hd;
  std::memset(&hd, 0, sizeof(hd));
  std::memcpy(hd.magic, "RMXSTATE", 8);
  hd.version = kStateVersion;
  hd.has_rng = has_rng ? 1u : 0u;
  hd.n_agents = h->cfg.n_agents;
  hd.n_envs = h->cfg.n_envs;
  hd.base_seed = h->base_seed;
  hd.digest = h->digest;
  hd.env_offset = h->cfg.env_offset;
  hd.n_envs_global = h->cfg.n_envs_global;
  if (h->host) {
    std::memcpy(hd.stats, h->host->stats, sizeof(hd.stats));
  } else {
    HIP_TRY(reduce_stats(h, h->d_stats, nullptr), "stats launch");
    HIP_TRY(hipMemcpy(hd.stats, h->d_stats, sizeof(hd.stats), hipMemcpyDeviceToHost), "stats copy");
  }
  unsigned char* dst = static_cast<unsigned char*>(host_blob);
  std::memcpy(dst, &hd, sizeof(hd));
  dst += sizeof(hd);
  for (const auto& c : cols) {
    if (h->host)
      std::memcpy(dst, c.dev, c.bytes);
    else
      HIP_TRY(hipMemcpy(dst, c.dev, c.bytes, hipMemcpyDeviceToHost), "get_state copy");
    dst += c.bytes;
  }
  return RMX_OK;
}

int rmx_set_state(rmx_handle* h, const void* host_blob, size_t bytes) {
  int rc = check_bound(h);
  if (rc) return rc;
  std::vector<StateCol> cols;
  bool has_rng = false;
  state_columns(h, cols, has_rng);
  if (!host_blob || bytes != state_blob_bytes(cols)) return fail(RMX_E_INVALID, "state blob NULL or of the wrong size");
  StateHeader hd;
  std::memcpy(&hd, host_blob, sizeof(hd));
  if (std::memcmp(hd.magic, "RMXSTATE", 8) != 0 || hd.version != kStateVersion)
    return fail(RMX_E_INVALID, "not an rmx state blob of this version");
  if (hd.n_agents != h->cfg.n_agents || hd.n_envs != h->cfg.n_envs || hd.has_rng != (has_rng ? 1u : 0u))
    return fail(RMX_E_INVALID, "state blob shape (agents, envs, rng columns) differs from the handle");
  if (hd.digest != h->digest)
    return fail(RMX_E_INVALID, "state blob was written by a handle of another scenario (map, rules, RM or slip tables)");
  if (hd.env_offset != h->cfg.env_offset || hd.n_envs_global != h->cfg.n_envs_global)
    return fail(RMX_E_INVALID, "state blob was written for another shard (env_offset / n_envs_global)");
  {  // the columns index the tables: every cell, RM state and timestep must be in range before the upload
    const size_t AN = (size_t)h->cfg.n_agents * h->cfg.n_envs, N = (size_t)h->cfg.n_envs;
    const unsigned char* c0 = static_cast<const unsigned char*>(host_blob) + sizeof(hd);
    auto col = [&](int k, size_t i) {
      int32_t v;
      std::memcpy(&v, c0 + (size_t)k * 4 * AN + 4 * i, 4);
      return v;
    };
    for (size_t i = 0; i < AN; ++i)
      if ((uint32_t)col(0, i) >= (uint32_t)h->cfg.width || (uint32_t)col(1, i) >= (uint32_t)h->cfg.height ||
          (uint32_t)col(2, i) >= (uint32_t)h->cfg.n_rm_states)
        return fail(RMX_E_INVALID, "state blob holds a cell or RM state outside the handle's tables");
    for (size_t e = 0; e < N; ++e) {
      int32_t t;
      std::memcpy(&t, c0 + 5 * 4 * AN + 4 * e, 4);
      if (t < 0) return fail(RMX_E_INVALID, "state blob holds a negative timestep");
    }
  }
  if (h->host) {
    const unsigned char* src = static_cast<const unsigned char*>(host_blob) + sizeof(hd);
    for (const auto& c : cols) {
      std::memcpy(c.dev, src, c.bytes);
      src += c.bytes;
    }
    h->base_seed = h->host->base_seed = hd.base_seed;
    std::memcpy(h->host->stats, hd.stats, sizeof(hd.stats));
    h->host->traces_clear(nullptr);  // the Q(lambda) lists are not in the blob: the restored envs start without traces
    return RMX_OK;
  }
  SYNC_END_OR_RETURN(h);
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  HIP_TRY(hipDeviceSynchronize(), "sync before set_state");
  const unsigned char* src = static_cast<const unsigned char*>(host_blob) + sizeof(hd);
  for (const auto& c : cols) {
    HIP_TRY(hipMemcpy(c.dev, src, c.bytes, hipMemcpyHostToDevice), "set_state copy");
    src += c.bytes;
  }
  h->base_seed = hd.base_seed;
  h->rs_dirty = true;  // the restored rng columns are the blob's
  // statistics: cleared, then the saved totals placed in slab slot 0 (every report sums the whole slab)
  HIP_TRY(hipMemset(h->d_slab, 0, sizeof(double) * RMX_NSTATS * h->n_waves), "stats clear");
  if (h->d_es) HIP_TRY(hipMemset(h->d_es, 0, h->es_bytes), "stats clear");
  HIP_TRY(hipMemcpy(h->d_slab, hd.stats, sizeof(hd.stats), hipMemcpyHostToDevice), "stats restore");
  HIP_TRY(refresh_starts(h, nullptr), "restore start cache / precompute");  // the restored base seed's
  // the Q(lambda) lists are not in the blob: the restored envs start without traces
  if ((rc = lambda_clear(h, nullptr, nullptr))) return rc;
  HIP_TRY(hipDeviceSynchronize(), "sync after set_state");
  return RMX_OK;
}

}  // extern "C"
