// ivox_map.hpp -- the device iVox as the other units of the GICP family see it: the map object (ivox.hip creates, fills and sweeps it) and its
// description as a target of the factor kernels (gicp.hip's factors, gicp_align.hip's batches and ct_align.hip's loop run over gicp_target(map)).
#pragma once
#include <atomic>
#include <cstdint>

#include "gicp_factor.hpp"

struct glim_amd_ivox {
  CtxRef ctx;
  double leaf = 1.0, inv_leaf = 1.0;
  double min_dist = 0.1;                      // FlatContainer::Setting::min_sq_dist_in_cell = min_dist^2
  int cap = 20;                               // max_num_points_in_cell (1..64: a cell never holds more than one wavefront's lanes)
  int lru_horizon = 10, lru_clear_cycle = 10, lru_counter = 0;
  int mode = 7;                               // neighbour voxel mode of the search
  int num_slots = 0;                          // voxels
  int64_t num_points = 0;
  int slot_cap = 0, init_slots = 1024;
  unsigned int tsize = 0;                     // table entries (power of two), 0 before the first insert
  unsigned long long* tkeys = nullptr;
  int* tslots = nullptr;
  unsigned long long* skey = nullptr;         // per slot
  int* scount = nullptr;
  int* slru = nullptr;
  float4* pts = nullptr;                      // slot_cap * cap
  float4* covA = nullptr;
  float2* covB = nullptr;
  uint64_t generation = 1;                    // moves with every insert: what a factor's kept correspondences are checked against
  std::atomic<int> live_factors{0};           // continuous-time factors built on the map; destroy is refused while one lives
};

namespace {

constexpr int64_t IVOX_MAX_SOURCE = 1 << 28;  // source points of a rigid factor over the map

// the map as a target of the factor kernels (GicpTarget), as it is now
GicpTarget gicp_target(const glim_amd_ivox* m, bool lock = true) {
  GicpTarget t;
  if (!m) return t;
  t.ctx = m->ctx;
  if (lock) t.held = std::unique_lock<std::mutex>(t.ctx->mu);
  t.args.sorted = m->pts;
  t.args.tA = m->covA;
  t.args.tB = m->covB;
  t.args.nt = (int)m->num_points;
  t.args.h = m->leaf;
  t.args.inv_h = m->inv_leaf;
  t.ivox = true;
  t.nn.keys = m->tkeys;
  t.nn.slots = m->tslots;
  t.nn.counts = m->scount;
  t.nn.mask = m->tsize - 1;
  t.nn.cap = m->cap;
  t.nn.nnb = m->mode;
  t.nn.inv_leaf = m->inv_leaf;
  t.empty = m->num_slots == 0;
  t.max_source = IVOX_MAX_SOURCE;
  t.generation = m->generation;
  return t;
}

}  // namespace
