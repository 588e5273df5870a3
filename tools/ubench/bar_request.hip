// bar_request.hip -- can the HOST post a request straight into DEVICE memory (large BAR) instead of leaving it in host memory for the resident
// kernel's leader to fetch with PCIe READS?  (the request side of the synchronous call is a PCIe read round trip, ~1.2 us, polled.)
//   hipcc -O3 --offload-arch=gfx950 tools/ubench/bar_request.hip -o /tmp/bar_request && /tmp/bar_request
// A 1-block resident kernel polls a request word and answers by writing the sequence number into a host-mapped completion word:
//   host_word      the request word lives in pinned host memory (what vgicp.hip's resident session does): the kernel polls over PCIe
//   device_word    the request word lives in fine-grained DEVICE memory (hipExtMallocWithFlags, hipDeviceMallocFinegrained) and the host stores
//                  into it through the same pointer -- works only where the device memory is host-visible (large BAR); the program reports and
//                  skips the row when the allocation or the first host store is refused
// Prints the median round trip of 2000 requests after 200 warm-ups.
//
// Session-shaped rows (responder_kernel): does the request reach ALL the blocks of a resident session sooner when the host writes the pose
// granules itself?  W = 256 blocks of 256 threads (and W + 1); lanes 0..11 of wave 0 of every block poll the 12 granules of replica
// blockIdx % R with the session's back-off (vgicp.hip wait_pose); ONE chosen block answers into the host-mapped completion word.
//   lines    today's path: the last block leads -- it polls one 64-byte line in pinned host memory and re-publishes R x 12 granules
//            {lo, hi, tag, 0} in device memory with write-through stores; everyone (the leader too) then sees them with agent-scope loads
//   direct   the host stores the R x 12 granules {lo, tag, hi, tag} itself, as aligned 8-byte halves through the large BAR into fine-grained
//            device memory, one sfence behind the last; the blocks load at system scope and take a granule only when both tags agree
// For every R in {1, 2, 4, 8} the answering block is taken in turn from the first, the middle and the last index and one block of every
// blockIdx % 8 class; the row gives the median over those blocks of the median round trip (1000 requests after 200 warm-ups), and the slowest
// block's median.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <csetjmp>
#include <csignal>
#include <cstdio>
#include <vector>

#define CK(x)                                              \
  do {                                                     \
    hipError_t e = (x);                                    \
    if (e != hipSuccess) {                                 \
      printf("%s failed: %s\n", #x, hipGetErrorString(e)); \
      return 1;                                            \
    }                                                      \
  } while (0)

__global__ void poll_kernel(const unsigned int* request, unsigned int* completion, unsigned int idle_limit) {
  unsigned int last = 0;
  for (unsigned int idle = 0; idle < idle_limit; idle++) {
    const unsigned int r = __hip_atomic_load(request, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (r == 0xffffffffu) return;
    if (r != last) {
      last = r;
      idle = 0;
      __hip_atomic_store(completion, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __builtin_amdgcn_s_sleep(2);
  }
}

// The same responder with the poll spread over the four wavefronts of a 256-thread block: every wavefront keeps ONE read of the request word in
// flight, started a quarter of a round trip after its neighbour's, and the first to see a new value answers (LDS compare-and-swap).  The expected
// wait of a request for the next poll to START drops from half a read round trip to an eighth.
__global__ void poll_kernel_staggered(const unsigned int* request, unsigned int* completion, unsigned int idle_limit, int stagger_sleep) {
  __shared__ unsigned int s_last;
  if (threadIdx.x == 0) s_last = 0u;
  __syncthreads();
  if ((threadIdx.x & 63) != 0) return;
  const int wave = (int)threadIdx.x >> 6;
  for (int k = 0; k < wave * stagger_sleep; k++) __builtin_amdgcn_s_sleep(1);  // (64 cycles each: the s_sleep argument has to be a constant)
  for (unsigned int idle = 0; idle < idle_limit; idle++) {
    const unsigned int r = __hip_atomic_load(request, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (r == 0xffffffffu) return;
    const unsigned int last = __hip_atomic_load(&s_last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (r != last) {
      unsigned int expected = last;
      if (__hip_atomic_compare_exchange_strong(&s_last, &expected, r, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
        idle = 0;
        __hip_atomic_store(completion, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
    __builtin_amdgcn_s_sleep(2);
  }
}

// ---- session-shaped responder ---------------------------------------------------------------------------------------------------------
typedef int v4i_t __attribute__((ext_vector_type(4)));
constexpr unsigned int AUX_SC1 = 16u;                             // agent scope (vgicp.hip)
constexpr unsigned int AUX_SC1_VOLATILE = 16u | (1u << 31);
constexpr unsigned int AUX_SYS_VOLATILE = 17u | (1u << 31);       // sc0 sc1: system scope
constexpr unsigned int EXIT_TAG = 0xffffffffu;
constexpr int GRANULES = 12;

struct ResponderArgs {
  char* pose16;                      // R x 12 granules of 16 bytes
  int replicas;
  int direct;                        // 0: lines (a leader re-publishes), 1: the host wrote the granules
  const unsigned long long* h_line;  // lines: one 64-byte line {7 doubles, tag} in pinned host memory
  int answer_block;
  unsigned int* completion;          // host-mapped
  unsigned int leader_idle_polls, poll_limit;
};

__global__ __launch_bounds__(256) void responder_kernel(const ResponderArgs a) {
  __shared__ unsigned int s_tag;
  const int b = (int)blockIdx.x;
  const bool leader = !a.direct && b == (int)gridDim.x - 1;
  unsigned int last = 0u;
  for (;;) {
    if (leader) {
      // the session leader's loop: word w of the line is read by thread w, the tag is word 7
      unsigned int req = EXIT_TAG;
      unsigned long long w0 = 0ull;
      if (threadIdx.x < 64) {
        for (unsigned int idle = 0; idle < a.leader_idle_polls; idle++) {
          w0 = __hip_atomic_load(a.h_line + (threadIdx.x & 7), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          const unsigned int t = (unsigned int)__shfl((unsigned int)w0, 7, 64);
          if (t != last) {
            req = t;
            break;
          }
          __builtin_amdgcn_s_sleep(2);
        }
        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(a.pose16, 0, a.replicas * GRANULES * 16, 0x00020000);
        if (threadIdx.x < GRANULES) {
          const unsigned long long v = __shfl(w0, (int)(threadIdx.x % 7), 64);
          const v4i_t g = {(int)(v & 0xffffffffull), (int)(v >> 32), (int)req, 0};
          for (int c = 0; c < a.replicas; c++) __builtin_amdgcn_raw_buffer_store_b128(g, rsrc, (c * GRANULES + (int)threadIdx.x) * 16, 0, AUX_SC1);
        }
        if (threadIdx.x == 0) s_tag = req;
      }
      __syncthreads();
      if (s_tag == EXIT_TAG) return;
    }
    // wait_pose: lanes 0..11 of wave 0 poll the granules of this block's replica
    if (threadIdx.x < 64) {
      const int lane = (int)threadIdx.x < GRANULES ? (int)threadIdx.x : 0;
      const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(a.pose16 + (size_t)(b % a.replicas) * GRANULES * 16, 0, GRANULES * 16, 0x00020000);
      unsigned int tag = EXIT_TAG;
      for (unsigned int spins = 0; spins < a.poll_limit; spins++) {
        const v4i_t g = a.direct ? __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane * 16, 0, AUX_SYS_VOLATILE)
                                 : __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane * 16, 0, AUX_SC1_VOLATILE);
        const unsigned int t = a.direct ? (unsigned int)g.y : (unsigned int)g.z;
        const bool whole = a.direct ? g.y == g.w : true;  // direct: both halves of the granule carry the tag
        const bool mine = whole && t != 0u && t != last;
        const unsigned int t0 = (unsigned int)__builtin_amdgcn_readfirstlane((int)t);
        if (__all(mine && t == t0)) {
          tag = t0;
          break;
        }
        if (__any(whole && t == EXIT_TAG)) break;  // exit dominates
        if (spins < 32) __builtin_amdgcn_s_sleep(4);
        else if (spins < 256) __builtin_amdgcn_s_sleep(24);
        else __builtin_amdgcn_s_sleep(100);
      }
      if (threadIdx.x == 0) s_tag = tag;
    }
    __syncthreads();
    const unsigned int tag = s_tag;
    if (tag == EXIT_TAG) return;
    if (b == a.answer_block && threadIdx.x == 0) __hip_atomic_store(a.completion, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    last = tag;
    __syncthreads();
  }
}

// one session: launch, 1200 requests, exit.  Returns the median round trip in us, < 0 when a request was not answered within 2 s.
static double run_session(int direct, int blocks, int replicas, int answer_block, char* pose16_dev, volatile unsigned long long* pose16_host,
                          volatile unsigned long long* h_line, const unsigned long long* h_line_dev, volatile unsigned int* h_done, unsigned int* d_done,
                          hipStream_t st) {
  const int n = replicas * GRANULES;
  if (direct) {
    for (int i = 0; i < 2 * n; i++) pose16_host[i] = 0ull;
    __builtin_ia32_sfence();
  } else {
    if (hipMemsetAsync(pose16_dev, 0, (size_t)n * 16, st) != hipSuccess) return -1.0;
    for (int i = 0; i < 8; i++) h_line[i] = 0ull;
  }
  *h_done = 0;
  ResponderArgs a;
  a.pose16 = pose16_dev;
  a.replicas = replicas;
  a.direct = direct;
  a.h_line = h_line_dev;
  a.answer_block = answer_block;
  a.completion = d_done;
  a.leader_idle_polls = 1u << 20;  // (~1.5 s of empty polls: the host always ends the session itself)
  a.poll_limit = 1u << 19;
  responder_kernel<<<blocks, 256, 0, st>>>(a);
  if (hipGetLastError() != hipSuccess) return -1.0;
  std::vector<double> us;
  bool lost = false;
  auto post = [&](unsigned int tag, unsigned int s) {
    if (direct) {
      // every replica's granules: two aligned 8-byte halves {lo, tag} {hi, tag} each, one sfence behind the last
      for (int c = 0; c < replicas; c++)
        for (int i = 0; i < GRANULES; i++) {
          const unsigned long long v = 0x3ff0000000000000ull + s + (unsigned)i;
          pose16_host[2 * (c * GRANULES + i)] = (v & 0xffffffffull) | ((unsigned long long)tag << 32);
          pose16_host[2 * (c * GRANULES + i) + 1] = (v >> 32) | ((unsigned long long)tag << 32);
        }
    } else {
      for (int i = 0; i < 7; i++) h_line[i] = 0x3ff0000000000000ull + s + (unsigned)i;
      __asm__ volatile("" ::: "memory");
      h_line[7] = tag;
    }
    __builtin_ia32_sfence();
  };
  unsigned int s = 0;
  for (int i = 0; i < 1200 && !lost; i++) {
    const auto t0 = std::chrono::steady_clock::now();
    ++s;
    post(0x80000000u | s, s);
    unsigned long spins = 0;
    while (*h_done != (0x80000000u | s)) {
      __builtin_ia32_pause();
      if ((++spins & 0xfffff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
        lost = true;
        break;
      }
    }
    const double dt = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (i >= 200) us.push_back(dt);
  }
  post(EXIT_TAG, 0);
  if (hipStreamSynchronize(st) != hipSuccess || lost) return -1.0;
  std::sort(us.begin(), us.end());
  return us[us.size() / 2];
}

static sigjmp_buf g_jmp;
static void on_segv(int) { siglongjmp(g_jmp, 1); }

static double run(volatile unsigned int* request_host_view, const unsigned int* request_dev, volatile unsigned int* h_done, unsigned int* d_done, hipStream_t st, int stagger = -1) {
  *request_host_view = 0;
  *h_done = 0;
  if (stagger < 0) poll_kernel<<<1, 64, 0, st>>>(request_dev, d_done, 1u << 22);
  else poll_kernel_staggered<<<1, 256, 0, st>>>(request_dev, d_done, 1u << 22, stagger);
  std::vector<double> us;
  unsigned int s = 0;
  for (int i = 0; i < 2200; i++) {
    const auto t0 = std::chrono::steady_clock::now();
    *request_host_view = ++s;
    __builtin_ia32_sfence();
    unsigned long spins = 0;
    while (*h_done != s && ++spins < (1ul << 28)) __builtin_ia32_pause();
    const double dt = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (i >= 200) us.push_back(dt);
  }
  *request_host_view = 0xffffffffu;
  __builtin_ia32_sfence();
  (void)hipStreamSynchronize(st);
  std::sort(us.begin(), us.end());
  return us[us.size() / 2];
}

int main() {
  hipStream_t st;
  CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  unsigned int *h = nullptr, *d = nullptr;
  CK(hipHostMalloc(&h, 256, hipHostMallocMapped));
  CK(hipHostGetDevicePointer((void**)&d, h, 0));
  printf("host_word   (request polled over PCIe):      %.2f us per request\n", run(h, d, h + 16, d + 16, st));
  for (int stagger : {0, 4, 8, 12}) printf("host_word, four staggered wavefronts (s_sleep %2d between their first polls): %.2f us per request\n", stagger, run(h, d, h + 16, d + 16, st, stagger));
  printf("host_word   (again):                         %.2f us per request\n", run(h, d, h + 16, d + 16, st));
  unsigned int* fine = nullptr;
  hipError_t e = hipExtMallocWithFlags((void**)&fine, 256, hipDeviceMallocFinegrained);
  if (e != hipSuccess) {
    printf("device_word: hipExtMallocWithFlags(hipDeviceMallocFinegrained) refused: %s\n", hipGetErrorString(e));
    (void)hipGetLastError();
    return 0;
  }
  CK(hipMemset(fine, 0, 256));
  signal(SIGSEGV, on_segv);
  signal(SIGBUS, on_segv);
  if (sigsetjmp(g_jmp, 1)) {
    printf("device_word: the host cannot store into device memory through this pointer (no large BAR mapping): not available here\n");
    return 0;
  }
  *(volatile unsigned int*)fine = 0;  // faults where the memory is not host-visible
  printf("device_word (request stored through the BAR): %.2f us per request\n", run(fine, fine, h + 16, d + 16, st));

  // ---- session-shaped rows
  constexpr int W = 256;
  char *pose_plain = nullptr, *pose_fine = nullptr;
  CK(hipMalloc((void**)&pose_plain, 8 * GRANULES * 16));
  CK(hipExtMallocWithFlags((void**)&pose_fine, 8 * GRANULES * 16, hipDeviceMallocFinegrained));
  CK(hipMemset(pose_fine, 0, 8 * GRANULES * 16));
  CK(hipDeviceSynchronize());
  printf("session-shaped responder: blocks of 256 threads, 12 granules per replica, answering block in turn first / middle / last / one per blockIdx %% 8 class\n");
  printf("%-7s %6s %3s  %10s %10s   per answering block (us)\n", "variant", "blocks", "R", "median_us", "slowest_us");
  for (int blocks : {W, W + 1})
    for (int R : {1, 2, 4, 8})
      for (int direct = 0; direct < 2; direct++) {
        std::vector<int> answer = {0, blocks / 2, blocks - 1};
        for (int k = 0; k < 8; k++) answer.push_back(64 + 8 + k);  // block 72 + k: class k
        std::vector<double> med;
        for (int ab : answer) {
          const double m = run_session(direct, blocks, R, ab, direct ? pose_fine : pose_plain, (volatile unsigned long long*)pose_fine, (volatile unsigned long long*)(h + 32),
                                       (const unsigned long long*)(d + 32), h + 16, d + 16, st);
          if (m < 0.0) {
            printf("%-7s %6d %3d  answering block %d: a request was not answered -- stopping\n", direct ? "direct" : "lines", blocks, R, ab);
            return 1;
          }
          med.push_back(m);
        }
        std::vector<double> sorted = med;
        std::sort(sorted.begin(), sorted.end());
        printf("%-7s %6d %3d  %10.2f %10.2f  ", direct ? "direct" : "lines", blocks, R, sorted[sorted.size() / 2], sorted.back());
        for (size_t i = 0; i < med.size(); i++) printf(" %d:%.2f", answer[i], med[i]);
        printf("\n");
        fflush(stdout);
      }
  return 0;
}
