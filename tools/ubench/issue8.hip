// gfx950 issue cost of the slice kernel's select, lane-read and wrap forms (round 9), in the
// harness of issue3.hip: 8 independent chains per wave, 12 waves per CU (3 per SIMD, the slice
// kernel's occupancy); prints SIMD cycles per wave-instruction at 2.4 GHz (compare rows).
// Also checks that v_pk_mul_f32 honours op_sel / op_sel_hi on an SGPR-pair source.
//   hipcc --offload-arch=gfx950 -O2 tools/ubench/issue8.hip -o tools/ubench/issue8
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>

#define BODY(NAME, ASM)                                                                   \
  __global__ void k_##NAME(uint32_t* out, int iters) {                                   \
    uint32_t a[8], b[8], t[8] = {0, 0, 0, 0, 0, 0, 0, 0};                                \
    const uint32_t s = out[1024];                                                        \
    const uint64_t s64 = ((uint64_t)(s ^ 0x55555555u) << 32) | s;                        \
    uint32_t m = (threadIdx.x >> 3) & 1 ? ~0u : 0u;                                      \
    asm volatile("" : "+v"(m));                                                          \
    for (int j = 0; j < 8; j++) { a[j] = threadIdx.x * 7 + j; b[j] = threadIdx.x ^ (j * 977); } \
    for (int it = 0; it < iters; it++) {                                                 \
      _Pragma("unroll") for (int j = 0; j < 8; j++) { ASM; }                              \
    }                                                                                    \
    uint32_t r = (uint32_t)s64 ^ m;                                                      \
    for (int j = 0; j < 8; j++) r ^= a[j] ^ b[j] ^ t[j];                                 \
    if (r == 0x1234) out[threadIdx.x] = r;                                               \
  }

#define A0 "+v"(a[j])
BODY(xor_v, asm volatile("v_xor_b32 %0, %1, %0" : A0 : "v"(b[j])))
BODY(cndmask_vcc, asm volatile("v_cndmask_b32 %0, %0, %1, vcc" : A0 : "v"(b[j])))
BODY(cndmask_e64_sgpr, asm volatile("v_cndmask_b32_e64 %0, %0, %1, %2" : A0 : "v"(b[j]), "s"(s64)))
BODY(bitop3_ca_vmask, asm volatile("v_bitop3_b32 %0, %2, %0, %1 bitop3:0xca" : A0 : "v"(b[j]), "v"(m)))
BODY(readlane, asm volatile("v_readlane_b32 %0, %1, 5" : "=s"(t[j]) : "v"(a[j])))
BODY(min_u32, asm volatile("v_min_u32 %0, %1, %0" : A0 : "v"(b[j])))
BODY(pk_mul_vgpr, asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(*(uint64_t*)&a[j & 6]) : "v"(*(uint64_t*)&b[j & 6])))
BODY(pk_mul_sgpr, asm volatile("v_pk_mul_f32 %0, %1, %0" : "+v"(*(uint64_t*)&a[j & 6]) : "s"(s64)))
BODY(pk_mul_sgpr_opsel, asm volatile("v_pk_mul_f32 %0, %1, %0 op_sel:[1,0] op_sel_hi:[1,1]" : "+v"(*(uint64_t*)&a[j & 6]) : "s"(s64)))

// {2, 3} in an SGPR pair times {5, 7}: the low half for both lanes, then the high half
__global__ void k_opsel_check(float* out) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  const uint64_t gg = ((uint64_t)__float_as_uint(out[9]) << 32) | __float_as_uint(out[8]);
  const f2 z = {out[10], out[11]};
  f2 lo, hi;
  asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(lo) : "s"(gg), "v"(z));
  asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(hi) : "s"(gg), "v"(z));
  if (threadIdx.x == 0) { out[0] = lo.x; out[1] = lo.y; out[2] = hi.x; out[3] = hi.y; }
}

typedef void (*K)(uint32_t*, int);
int main() {
  uint32_t* out;
  (void)hipMalloc(&out, 1 << 20);
  (void)hipMemset(out, 0, 1 << 20);
  const float in[4] = {2.0f, 3.0f, 5.0f, 7.0f};
  float res[4] = {0, 0, 0, 0};
  (void)hipMemcpy(out + 8, in, sizeof(in), hipMemcpyHostToDevice);
  hipLaunchKernelGGL(k_opsel_check, dim3(1), dim3(64), 0, 0, (float*)out);
  (void)hipMemcpy(res, out, sizeof(res), hipMemcpyDeviceToHost);
  const bool ok = res[0] == 10.0f && res[1] == 14.0f && res[2] == 15.0f && res[3] == 21.0f;
  printf("pk_mul op_sel on an SGPR pair {2,3} x {5,7}: low half %g %g, high half %g %g  %s\n", res[0], res[1], res[2],
         res[3], ok ? "OK" : "WRONG");
  (void)hipMemset(out, 0, 64);
  int cus = 0;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
#define E(n, i) {#n, k_##n, i}
  struct { const char* n; K k; int instrs; } ks[] = {
      E(xor_v, 1), E(cndmask_vcc, 1), E(cndmask_e64_sgpr, 1), E(bitop3_ca_vmask, 1), E(readlane, 1), E(min_u32, 1),
      E(pk_mul_vgpr, 1), E(pk_mul_sgpr, 1), E(pk_mul_sgpr_opsel, 1)};
  hipEvent_t a, b;
  (void)hipEventCreate(&a);
  (void)hipEventCreate(&b);
  const int iters = 20000;
  const int wpc = 12;
  for (auto& e : ks) {
    const int threads = 256, blocks = cus * wpc / 4;
    float ms = 0;
    for (int rep = 0; rep < 2; rep++) {
      (void)hipEventRecord(a);
      hipLaunchKernelGGL(e.k, dim3(blocks), dim3(threads), 0, 0, out, iters);
      (void)hipEventRecord(b);
      (void)hipEventSynchronize(b);
      (void)hipEventElapsedTime(&ms, a, b);
    }
    const double per_simd = (double)iters * 8 * e.instrs * (blocks * threads / 64) / cus / 4;
    printf("waves/CU %2d  %-20s %8.3f ms  %.3f cyc/wave-instr/SIMD @2.4GHz\n", wpc, e.n, ms,
           ms * 1e-3 * 2.4e9 / per_simd);
  }
  return ok ? 0 : 1;
}
