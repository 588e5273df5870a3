// row_handoff.hip -- how fast a finalising block of the resident session can HOLD the tagged rows of a request, by the form of its poll.
// Session-shaped: ONE persistent launch of R producer blocks, the consumer blocks, 32 "chain" blocks and a leader; a round begins when the
// host bumps a tag in host-mapped memory (the leader re-publishes it in device memory, 8 replicas, as the pose granules are).  A producer
// waits BASE + a per-block, per-round pseudo-random 0..1.2 us (the spread of the real workers' publication: 2.71..3.92 us after the pose),
// publishes ten {3 floats, tag} granules of its row with ONE sc1 16-byte store instruction (vgicp.hip publish_row_tagged) and stamps
// s_memrealtime; a consumer stamps once its block holds every granule it owns (behind a block barrier) and tells the host.
//   hipcc -O3 --offload-arch=gfx950 tools/ubench/row_handoff.hip -o /tmp/row_handoff && timeout -k 10 120 /tmp/row_handoff
// Prints, per R = 16 / 128 / 256 and per form, over 2000 rounds after 200 warm-up: (latest consumer stamp - latest producer stamp) in us
// -- median, 5 / 25 / 75 / 95th percentile --, the host's round trip, and the round time of the 32 chain blocks (a dependent chain of plain
// loads through a 4 MB table: does a faster-polling form slow the workers?).
//   A          today's fused_finalize<8>: ONE 256-thread block, thread k owns (group, piece) pairs k and k + 256 of 320, batches of 8 or
//              2 x 8 loads, all-or-nothing, s_sleep(4) between sweeps
//   B(K)       ten consumer blocks, one per piece p; thread r owns granule p of row r and keeps K loads of it in flight, issued a fixed
//              s_sleep apart; the oldest is examined behind a counted wait; a lane that holds its granule stops issuing
//   B(K) s/f   the same, but one load at a time with s_sleep(24) until any lane of the wavefront has seen the tag, then B(K)
// Every spin is bounded; a lost round is reported, not waited for.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                              \
  do {                                                     \
    hipError_t e = (x);                                    \
    if (e != hipSuccess) {                                 \
      printf("%s failed: %s\n", #x, hipGetErrorString(e)); \
      return 1;                                            \
    }                                                      \
  } while (0)

typedef int v4i __attribute__((ext_vector_type(4)));
constexpr unsigned int SC1 = 16u, SC1_VOL = 16u | (1u << 31);
constexpr unsigned int EXIT_TAG = 0xffffffffu;
constexpr int BLOCK = 256, PIECES = 10, ROW_BYTES = PIECES * 16, GROUPS = 32, CHAIN_BLOCKS = 32, REPLICAS = 8;
constexpr int MAX_R = 256, MAX_ROUNDS = 2200, MAX_CONS = 16, CHAIN_STEPS = 6;
constexpr unsigned int TABLE_WORDS = 1u << 20;
constexpr unsigned int LOST_SPINS = 1u << 20;

struct Args {
  volatile unsigned int* req;   // host-mapped: the round's tag (host writes)
  unsigned int* done;           // host-mapped: done[16 c] = tag once consumer block c holds its granules
  unsigned int* go;             // device: REPLICAS x 16 words, the tag re-published by the leader
  char* rows;                   // device: R x ROW_BYTES
  unsigned long long* prod_stamp;  // [round][MAX_R]
  unsigned long long* cons_stamp;  // [round][MAX_CONS]
  unsigned int* chain_ticks;       // [round][CHAIN_BLOCKS]
  unsigned int* lost;              // consumers that gave up
  const unsigned int* table;       // TABLE_WORDS: the chain blocks' pointer chase
  float* sink;
  int R, ncons;
  unsigned int first_tag, base_ticks;
};

// thread 0 waits for a tag other than `last` in its replica of the go words; everyone gets it.  EXIT_TAG when the wait gives up.
__device__ __forceinline__ unsigned int wait_go(const Args& a, unsigned int last, unsigned int* s_word) {
  if (threadIdx.x == 0) {
    unsigned int t = EXIT_TAG;
    const unsigned int* w = a.go + 16 * (blockIdx.x % REPLICAS);
    for (unsigned int spins = 0; spins < (1u << 24); spins++) {
      const unsigned int v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (v != last && v != 0u) {
        t = v;
        break;
      }
      if (spins < 32) __builtin_amdgcn_s_sleep(4);
      else if (spins < 256) __builtin_amdgcn_s_sleep(24);
      else __builtin_amdgcn_s_sleep(100);
    }
    *s_word = t;
  }
  __syncthreads();
  const unsigned int t = *s_word;
  __syncthreads();
  return t;
}

// form A: fused_finalize<8> of vgicp.hip, sums kept in FP32 (only the polling matters here)
__device__ __forceinline__ bool consume_block_a(const Args& a, int seq, float* acc) {
  constexpr int INFLIGHT = 8;
  const int nb = a.R;
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(a.rows, 0, nb * ROW_BYTES, 0x00020000);
  const int kA = (int)threadIdx.x, kB = (int)threadIdx.x + BLOCK;
  const bool hasB = kB < GROUPS * PIECES;
  const int gA = kA / PIECES, pA = kA - gA * PIECES;
  const int gB = hasB ? kB / PIECES : gA, pB = hasB ? kB - gB * PIECES : pA;
  float s = 0.f;
  bool lost = false;
  for (int base = 0;; base += GROUPS * INFLIGHT) {
    const int cA = gA + base, cB = gB + base;
    const bool moreA = cA < nb, moreB = hasB && cB < nb;
    if (!moreA && !moreB) break;
    v4i va[INFLIGHT], vb[INFLIGHT];
    bool okA = !moreA, okB = !moreB;
    for (unsigned int spins = 0;; spins++) {
      if (!okA) {
        bool ok = true;
#pragma unroll
        for (int u = 0; u < INFLIGHT; u++) va[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, min(cA + GROUPS * u, nb - 1) * ROW_BYTES + pA * 16, 0, SC1_VOL);
        if (!okB) {
#pragma unroll
          for (int u = 0; u < INFLIGHT; u++) vb[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, min(cB + GROUPS * u, nb - 1) * ROW_BYTES + pB * 16, 0, SC1_VOL);
        }
#pragma unroll
        for (int u = 0; u < INFLIGHT; u++) ok = ok && va[u].w == seq;
        okA = ok;
        if (!okB) {
          bool okb = true;
#pragma unroll
          for (int u = 0; u < INFLIGHT; u++) okb = okb && vb[u].w == seq;
          okB = okb;
        }
      } else if (!okB) {
        bool okb = true;
#pragma unroll
        for (int u = 0; u < INFLIGHT; u++) {
          vb[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, min(cB + GROUPS * u, nb - 1) * ROW_BYTES + pB * 16, 0, SC1_VOL);
          okb = okb && vb[u].w == seq;
        }
        okB = okb;
      }
      if (okA && okB) break;
      if (spins > LOST_SPINS) {
        lost = true;
        break;
      }
      __builtin_amdgcn_s_sleep(4);
    }
    if (lost) break;
    if (moreA) {
#pragma unroll
      for (int u = 0; u < INFLIGHT; u++)
        if (cA + GROUPS * u < nb) s += __int_as_float(va[u].x) + __int_as_float(va[u].y) + __int_as_float(va[u].z);
    }
    if (moreB) {
#pragma unroll
      for (int u = 0; u < INFLIGHT; u++)
        if (cB + GROUPS * u < nb) s += __int_as_float(vb[u].x) + __int_as_float(vb[u].y) + __int_as_float(vb[u].z);
    }
  }
  *acc = s;
  return lost;
}

__device__ __forceinline__ void ring_load(v4i& v, int off, const v4i& rs) {
  asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen sc0 sc1" : "=&v"(v) : "v"(off), "s"(rs) : "memory");
}
template <int LEFT>
__device__ __forceinline__ void ring_wait(v4i& v) {
  asm volatile("s_waitcnt vmcnt(%1)" : "+v"(v) : "n"(LEFT) : "memory");
}

// form B(K): this block owns piece p, thread r granule p of row r
template <int K, int SLEEP, bool SLOWFAST>
__device__ __forceinline__ bool consume_block_b(const Args& a, int p, int seq, float* acc) {
  const int r = (int)threadIdx.x, R = a.R;
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(a.rows, 0, R * ROW_BYTES, 0x00020000);
  const bool mine = r < R;
  const int off = (mine ? r : 0) * ROW_BYTES + p * 16;
  bool have = !mine;
  v4i val = {0, 0, 0, 0};
  unsigned int spins = 0;
  if (SLOWFAST) {
    // nothing can have arrived yet: one load at a time, far apart, until the first lane of this wavefront sees the round's tag
    for (; spins < LOST_SPINS; spins++) {
      bool seen = false;
      if (!have) {
        const v4i v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, SC1_VOL);
        if (v.w == seq) {
          have = seen = true;
          val = v;
        }
      }
      if (__any(seen) || __all(have)) break;
      __builtin_amdgcn_s_sleep(24);
    }
  }
  if (!__all(have)) {
    // The ring is issued and awaited in assembly: the compiler's own wait in front of a load's first use is vmcnt(0) here (the uses sit
    // behind lane-dependent branches), which would wait for the YOUNGEST load of the ring every time.  A lane that holds its granule
    // moves its offset past the descriptor's range: such a load returns zeros without a memory request, and no branch is needed.
    const v4i rs = {(int)(unsigned int)((uintptr_t)a.rows & 0xffffffffu), (int)(unsigned int)(((uintptr_t)a.rows >> 32) & 0xffffu), R * ROW_BYTES, 0x00020000};
    constexpr int PAST = 0x7ffffff0;
    v4i v[K];
#pragma unroll
    for (int u = 0; u < K; u++) {
      ring_load(v[u], have ? PAST : off, rs);
      __builtin_amdgcn_s_sleep(SLEEP);
    }
    for (bool done = false; !done && spins < LOST_SPINS;) {
#pragma unroll
      for (int u = 0; u < K; u++) {
        // the oldest load of the ring (loads return in order: the counted wait leaves the K - 1 younger ones in flight)
        ring_wait<K - 1>(v[u]);
        if (!have && v[u].w == seq) {
          have = true;
          val = v[u];
        }
        if (__all(have)) {
          done = true;
          break;
        }
        ring_load(v[u], have ? PAST : off, rs);
        __builtin_amdgcn_s_sleep(SLEEP);
        spins++;
      }
    }
#pragma unroll
    for (int u = 0; u < K; u++) ring_wait<0>(v[u]);  // nothing of the ring lands in a register that has been given to something else
  }
  *acc = __int_as_float(val.x) + __int_as_float(val.y) + __int_as_float(val.z);
  return !__all(have);
}

// form: 0 = A, 1 / 2 / 4 = B(K), 12 / 14 = B(K) slow then fast
__global__ __launch_bounds__(BLOCK) void handoff_kernel(const Args a, int form) {
  __shared__ unsigned int s_word;
  __shared__ int s_lost;
  const int b = (int)blockIdx.x;
  const int cons0 = a.R, chain0 = a.R + a.ncons, leader = chain0 + CHAIN_BLOCKS;
  unsigned int last = a.first_tag;
  for (;;) {
    if (b == leader) {
      // ---- leader: the host's tag, re-published in device memory
      unsigned int t = EXIT_TAG;
      if (threadIdx.x == 0) {
        for (unsigned int idle = 0; idle < (1u << 21); idle++) {
          const unsigned int v = __hip_atomic_load((const unsigned int*)a.req, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          if (v != last) {
            t = v;
            break;
          }
          __builtin_amdgcn_s_sleep(2);
        }
        for (int c = 0; c < REPLICAS; c++) __hip_atomic_store(a.go + 16 * c, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      t = (unsigned int)__builtin_amdgcn_readfirstlane((int)t);
      if (threadIdx.x == 0) s_word = t;
      __syncthreads();
      t = s_word;
      __syncthreads();
      if (t == EXIT_TAG) return;
      last = t;
      continue;
    }
    const unsigned int tag = wait_go(a, last, &s_word);
    if (tag == EXIT_TAG) return;
    last = tag;
    const unsigned int round = tag - a.first_tag - 1u;
    if (round >= (unsigned int)MAX_ROUNDS) return;
    if (b < cons0) {
      // ---- producer: the workers' spread, then the row as ten granules by one store instruction, then the stamp
      if (threadIdx.x < 64) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        unsigned int h = (unsigned int)b * 2654435761u ^ (round * 40503u + 0x9e3779b9u);
        h ^= h >> 15;
        h *= 2246822519u;
        h ^= h >> 13;
        const unsigned long long wait = a.base_ticks + (h % 121u);  // 100 MHz ticks: 0..1.2 us
        for (int i = 0; i < 4096 && __builtin_amdgcn_s_memrealtime() - t0 < wait; i++) __builtin_amdgcn_s_sleep(1);
        if (threadIdx.x < PIECES) {
          const v4i piece = {__float_as_int(1.f + (float)threadIdx.x), __float_as_int(2.f), __float_as_int((float)b), (int)tag};
          const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(a.rows + (size_t)b * ROW_BYTES, 0, ROW_BYTES, 0x00020000);
          __builtin_amdgcn_raw_buffer_store_b128(piece, rsrc, (int)threadIdx.x * 16, 0, SC1);
        }
        if (threadIdx.x == 0) a.prod_stamp[(size_t)round * MAX_R + b] = __builtin_amdgcn_s_memrealtime();
      }
      continue;
    }
    if (b >= chain0) {
      // ---- chain block: a dependent chain of plain loads, timed
      if (threadIdx.x < 64) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        unsigned int i = ((unsigned int)(b - chain0) * 64u + threadIdx.x) * 4099u + round * 131u;
#pragma unroll 1
        for (int s = 0; s < CHAIN_STEPS; s++) i = a.table[i & (TABLE_WORDS - 1u)];
        if (i == 0xdeadbeefu) a.sink[0] = 1.f;
        const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
        if (threadIdx.x == 0) a.chain_ticks[(size_t)round * CHAIN_BLOCKS + (b - chain0)] = (unsigned int)(t1 - t0);
      }
      continue;
    }
    // ---- consumer
    const int c = b - cons0;
    float acc = 0.f;
    bool lost;
    if (form == 0) lost = consume_block_a(a, (int)tag, &acc);
    else if (form == 1) lost = consume_block_b<1, 4, false>(a, c, (int)tag, &acc);
    else if (form == 2) lost = consume_block_b<2, 16, false>(a, c, (int)tag, &acc);
    else if (form == 4) lost = consume_block_b<4, 8, false>(a, c, (int)tag, &acc);
    else if (form == 12) lost = consume_block_b<2, 16, true>(a, c, (int)tag, &acc);
    else lost = consume_block_b<4, 8, true>(a, c, (int)tag, &acc);
    if (threadIdx.x == 0) s_lost = 0;
    __syncthreads();
    if (lost) s_lost = 1;
    if (acc == -12345.f) a.sink[1] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      a.cons_stamp[(size_t)round * MAX_CONS + c] = __builtin_amdgcn_s_memrealtime();
      if (s_lost) atomicAdd(a.lost, 1u);
      __hip_atomic_store(a.done + 16 * c, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __syncthreads();
  }
}

static double pct(std::vector<double>& v, double q) {
  if (v.empty()) return 0.0;
  std::sort(v.begin(), v.end());
  return v[std::min(v.size() - 1, (size_t)(q * (double)v.size()))];
}

int main(int argc, char** argv) {
  const unsigned int base_ticks = argc > 1 ? (unsigned int)atoi(argv[1]) : 270u;  // 2.7 us: nothing is published earlier in a real request
  const int warm = 200, iters = 2000, rounds = warm + iters;
  hipStream_t st;
  CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  unsigned int *h = nullptr, *hd = nullptr;
  CK(hipHostMalloc(&h, 4096, hipHostMallocMapped));
  CK(hipHostGetDevicePointer((void**)&hd, h, 0));
  for (int i = 0; i < 1024; i++) h[i] = 0;
  Args a;
  a.req = hd;            // word 0
  a.done = hd + 64;      // words 64 + 16 c
  volatile unsigned int* h_req = h;
  volatile unsigned int* h_done = h + 64;
  CK(hipMalloc(&a.go, REPLICAS * 64));
  CK(hipMalloc(&a.rows, MAX_R * ROW_BYTES));
  CK(hipMalloc(&a.prod_stamp, sizeof(unsigned long long) * MAX_ROUNDS * MAX_R));
  CK(hipMalloc(&a.cons_stamp, sizeof(unsigned long long) * MAX_ROUNDS * MAX_CONS));
  CK(hipMalloc(&a.chain_ticks, sizeof(unsigned int) * MAX_ROUNDS * CHAIN_BLOCKS));
  CK(hipMalloc(&a.lost, 64));
  CK(hipMalloc(&a.sink, 64));
  unsigned int* d_table = nullptr;
  CK(hipMalloc(&d_table, sizeof(unsigned int) * TABLE_WORDS));
  {
    std::vector<unsigned int> t(TABLE_WORDS);
    for (unsigned int i = 0; i < TABLE_WORDS; i++) t[i] = (i * 1664525u + 1013904223u) >> 7;
    CK(hipMemcpy(d_table, t.data(), sizeof(unsigned int) * TABLE_WORDS, hipMemcpyHostToDevice));
  }
  a.table = d_table;
  a.base_ticks = base_ticks;
  CK(hipMemset(a.rows, 0, MAX_R * ROW_BYTES));
  CK(hipMemset(a.go, 0, REPLICAS * 64));
  std::vector<unsigned long long> ps((size_t)MAX_ROUNDS * MAX_R), cs((size_t)MAX_ROUNDS * MAX_CONS);
  std::vector<unsigned int> ch((size_t)MAX_ROUNDS * CHAIN_BLOCKS);
  printf("row_handoff: producers wait %.2f us + 0..1.2 us; %d rounds after %d warm-up; us = (last consumer stamp - last producer stamp)\n",
         base_ticks * 0.01, iters, warm);
  unsigned int tag = 0;
  struct Form {
    int id;
    const char* name;
  };
  const Form forms[] = {{0, "A"}, {1, "B(1)"}, {2, "B(2)"}, {4, "B(4)"}, {12, "B(2) slow/fast"}, {14, "B(4) slow/fast"}, {0, "A again"}};
  for (int R : {16, 128, 256}) {
    for (const Form& f : forms) {
      a.R = R;
      a.ncons = f.id == 0 ? 1 : PIECES;
      a.first_tag = tag;
      CK(hipMemsetAsync(a.prod_stamp, 0, sizeof(unsigned long long) * MAX_ROUNDS * MAX_R, st));
      CK(hipMemsetAsync(a.cons_stamp, 0, sizeof(unsigned long long) * MAX_ROUNDS * MAX_CONS, st));
      CK(hipMemsetAsync(a.chain_ticks, 0, sizeof(unsigned int) * MAX_ROUNDS * CHAIN_BLOCKS, st));
      CK(hipMemsetAsync(a.lost, 0, 64, st));
      handoff_kernel<<<R + a.ncons + CHAIN_BLOCKS + 1, BLOCK, 0, st>>>(a, f.id);
      CK(hipGetLastError());
      std::vector<double> host_us;
      bool ok = true;
      for (int i = 0; i < rounds && ok; i++) {
        const auto t0 = std::chrono::steady_clock::now();
        *h_req = ++tag;
        for (int c = 0; c < a.ncons && ok; c++) {
          for (unsigned long s = 0; h_done[16 * c] != tag; s++) {
            __builtin_ia32_pause();
            if ((s & 0xffff) == 0xffff && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
              ok = false;
              break;
            }
          }
        }
        if (i >= warm) host_us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
      }
      *h_req = EXIT_TAG;
      CK(hipStreamSynchronize(st));
      // (the exit tag stays in the go words: the next launch's blocks must not take it for news -- cleared here, the next tag is fresh anyway)
      CK(hipMemset(a.go, 0, REPLICAS * 64));
      *h_req = tag;
      unsigned int lost = 0;
      CK(hipMemcpy(&lost, a.lost, 4, hipMemcpyDeviceToHost));
      CK(hipMemcpy(ps.data(), a.prod_stamp, sizeof(unsigned long long) * ps.size(), hipMemcpyDeviceToHost));
      CK(hipMemcpy(cs.data(), a.cons_stamp, sizeof(unsigned long long) * cs.size(), hipMemcpyDeviceToHost));
      CK(hipMemcpy(ch.data(), a.chain_ticks, sizeof(unsigned int) * ch.size(), hipMemcpyDeviceToHost));
      if (!ok) {
        printf("R=%3d %-15s host gave up waiting (lost %u)\n", R, f.name, lost);
        return 2;
      }
      std::vector<double> d, chain;
      for (int i = warm; i < rounds; i++) {
        unsigned long long p = 0, c = 0;
        for (int r = 0; r < R; r++) p = std::max(p, ps[(size_t)i * MAX_R + r]);
        for (int k = 0; k < a.ncons; k++) c = std::max(c, cs[(size_t)i * MAX_CONS + k]);
        if (p && c) d.push_back(((double)c - (double)p) * 0.01);
        for (int k = 0; k < CHAIN_BLOCKS; k++)
          if (ch[(size_t)i * CHAIN_BLOCKS + k]) chain.push_back(ch[(size_t)i * CHAIN_BLOCKS + k] * 0.01);
      }
      const double m = pct(d, 0.5);
      printf("R=%3d %-15s hand-off us: median %.2f  p5 %.2f  p25 %.2f  p75 %.2f  p95 %.2f  (n=%zu, lost %u) | host round %.2f | chain blocks %.2f (p95 %.2f, n=%zu)\n",
             R, f.name, m, pct(d, 0.05), pct(d, 0.25), pct(d, 0.75), pct(d, 0.95), d.size(), lost, pct(host_us, 0.5), pct(chain, 0.5),
             pct(chain, 0.95), chain.size());
      fflush(stdout);
    }
  }
  return 0;
}
