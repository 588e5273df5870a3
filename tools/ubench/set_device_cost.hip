// set_device_cost.hip -- what does the hipSetDevice at the head of every synchronous call cost when the device is current already, and would a
// check in front of it (hipGetDevice + compare) be cheaper?
//   hipcc -O3 --offload-arch=gfx950 tools/ubench/set_device_cost.hip -o /tmp/set_device_cost && /tmp/set_device_cost
// Prints nanoseconds per call, median of 9 runs of 1 000 000 calls each.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <vector>

template <class F>
static double median_ns(F f) {
  std::vector<double> v;
  for (int r = 0; r < 9; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < 1000000; i++) f();
    v.push_back(std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / 1e6);
  }
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main() {
  if (hipSetDevice(0) != hipSuccess || hipFree(nullptr) != hipSuccess) {
    printf("no device\n");
    return 1;
  }
  volatile int sink = 0;
  printf("hipSetDevice(current device):        %.1f ns\n", median_ns([&] { sink = sink + (int)hipSetDevice(0); }));
  printf("hipGetDevice + compare (the check):  %.1f ns\n", median_ns([&] {
           int d = -1;
           (void)hipGetDevice(&d);
           if (d != 0) sink = sink + (int)hipSetDevice(0);
         }));
  printf("steady_clock::now():                 %.1f ns\n", median_ns([&] { sink = sink + (int)(std::chrono::steady_clock::now().time_since_epoch().count() & 1); }));
  return 0;
}
