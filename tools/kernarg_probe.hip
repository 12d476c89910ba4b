// kernarg_probe.hip -- what the kernel-argument fetch costs a short kernel on this box: a dependent chain of launches
// on one stream of a kernel that cannot form its one load address before its arguments are in registers.  Built twice,
//   hipcc --offload-arch=gfx950 -O3 tools/kernarg_probe.hip -o /tmp/kp_plain
//   hipcc --offload-arch=gfx950 -O3 -mllvm -amdgpu-kernarg-preload-count=16 tools/kernarg_probe.hip -o /tmp/kp_preload
// the first fetches them with s_load + s_waitcnt lgkmcnt(0) (a cold scalar miss per launch: the host wrote the block
// just now), the second gets the first 14 dwords -- the six pointers, `off` and `n`: 16 user SGPRs less the kernarg
// pointer; `i2` / `i3` are still fetched with s_load, behind the load -- in SGPRs at wave launch where the firmware
// preloads (`.amdhsa_user_sgpr_kernarg_preload_length` in the -save-temps assembly says what the compiler asked for).
// The difference of the two "us/launch" columns is one kernarg round trip; no difference = the firmware does not preload.
// Used for profiles/r16_kernarg_preload_summary.md.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

// 6 pointers + 4 ints = 16 dwords, 14 of them preloaded.  One load (address = first pointer + an int), one store; the
// other arguments are used, so that none is dropped from the kernarg block: they select nothing at the values the
// host passes.
__global__ __launch_bounds__(256) void probe_kernel(const float* __restrict__ a, float* __restrict__ out,
                                                    const float* __restrict__ p2, const float* __restrict__ p3,
                                                    const float* __restrict__ p4, const float* __restrict__ p5, int off,
                                                    int n, int i2, int i3) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float v = a[off + i];
  if (i2 == i3) v += p2[i] + p3[i] + p4[i] + p5[i];   // never: i2 != i3
  out[i] = v + 1.f;
}

int main() {
  constexpr int NMAX = 1024 * 256, CHAIN = 400, REP = 5;
  float *x, *y;
  CHECK(hipMalloc(&x, (NMAX + 64) * sizeof(float)));
  CHECK(hipMalloc(&y, (NMAX + 64) * sizeof(float)));
  CHECK(hipMemset(x, 0, (NMAX + 64) * sizeof(float)));
  CHECK(hipMemset(y, 0, (NMAX + 64) * sizeof(float)));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  for (int blocks : {1, 32, 256, 512, 1024}) {
    const int n = blocks * 256;
    float best = 1e30f, sum = 0.f;
    for (int rep = 0; rep < REP + 1; ++rep) {   // rep 0: warm-up
      CHECK(hipDeviceSynchronize());
      CHECK(hipEventRecord(e0, 0));
      // launch k reads what launch k - 1 wrote: a dependent chain (x -> y -> x ...), as the step's six kernels are
      for (int k = 0; k < CHAIN; ++k)
        hipLaunchKernelGGL(probe_kernel, dim3(blocks), dim3(256), 0, 0, (k & 1) ? y : x, (k & 1) ? x : y, x, y, x, y,
                           k & 15, n, 1, 2);
      CHECK(hipEventRecord(e1, 0));
      CHECK(hipEventSynchronize(e1));
      CHECK(hipGetLastError());
      float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
      if (rep == 0) continue;
      const float us = ms * 1000.f / CHAIN;
      best = us < best ? us : best;
      sum += us;
    }
    printf("blocks %4d : %.3f us/launch (min of %d chains of %d), mean %.3f\n", blocks, best, REP, CHAIN, sum / REP);
  }
  float h = 0.f;
  CHECK(hipMemcpy(&h, x, sizeof(float), hipMemcpyDeviceToHost));
  printf("check x[0] = %.0f\n", h);   // keeps the chain observable
  return 0;
}
