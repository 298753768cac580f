// fks_kern_jump.h -- fks_jump_kernel: every (seed, chunk) generator window by GF(2) jump-ahead.
#pragma once
#include <hip/hip_runtime.h>

#include "fks_internal.h"
#include "fks_dev_mt.h"

namespace fks {
namespace {

// ------------------------------------------------------------------ jump kernel
// grid (nseeds, ceil(nchunks / chunks_per_wg)); block kJumpThreads (16 waves).
// LDS holds one phase of the seed's x words (below) at a 3-word offset, so that
// y = x + 1 is 16-byte aligned.  Each wave evaluates the jump
// of one chunk at a time: lane l < 63 owns window words w = 10l .. 10l+9 and sweeps
// the 19937 coefficients of c(t) = t^J mod phi four at a time (jump_quad_step10; the
// 2-bit pair step it replaced and the one-phase kernel are in git history (commit
// 9dd4861); A/B logs profiles/r04n_jump_quad_ab.log, r04x_jump_2phase_ab.log), keeping
// y[i + 10l .. i + 10l + 15] in a 16-register sliding window fed by two ds_read_b64
// per step:  acc[j] ^= y[i + d + 10l + j] & -c[i + d]   (d = 0..3, j = 0..9).
constexpr int kJumpXOff = 3;            // x at word 3 -> y = x + 1 at word 4 (16 B aligned)

// acc[j] ^= XOR over the set bits d of the wave-uniform 4-bit code of w[d + j] (j < 10):
// coefficients 4 at a time.  A binary tree of scalar bit tests picks one of 16 bodies
// (none, one v_xor_b32, one v_bitop3_b32, or two of them per word), so a random polynomial
// costs 1.25 VALU ops per word per 4 coefficients -- 0.3125 per coefficient against the
// pair step's 0.375 -- and 4 scalar tests instead of 2 x (1-3) compares.
__device__ __forceinline__ void jump_quad_step10(uint32_t (&acc)[10], const uint32_t (&w)[13], uint32_t code) {
  asm volatile(
      "s_bitcmp1_b32 %[c], 3\n"
      "s_cbranch_scc1 .Lqb3k8x%=\n"
      "s_bitcmp1_b32 %[c], 2\n"
      "s_cbranch_scc1 .Lqb2k4x%=\n"
      "s_bitcmp1_b32 %[c], 1\n"
      "s_cbranch_scc1 .Lqb1k2x%=\n"
      "s_bitcmp1_b32 %[c], 0\n"
      "s_cbranch_scc1 .Lqb0k1x%=\n"
      "s_branch .Lqendx%=\n"
      ".Lqb0k1x%=:\n"
      "v_xor_b32 %[a0], %[a0], %[w0]\n"
      "v_xor_b32 %[a1], %[a1], %[w1]\n"
      "v_xor_b32 %[a2], %[a2], %[w2]\n"
      "v_xor_b32 %[a3], %[a3], %[w3]\n"
      "v_xor_b32 %[a4], %[a4], %[w4]\n"
      "v_xor_b32 %[a5], %[a5], %[w5]\n"
      "v_xor_b32 %[a6], %[a6], %[w6]\n"
      "v_xor_b32 %[a7], %[a7], %[w7]\n"
      "v_xor_b32 %[a8], %[a8], %[w8]\n"
      "v_xor_b32 %[a9], %[a9], %[w9]\n"
      "s_branch .Lqendx%=\n"
      ".Lqb1k2x%=:\n"
      "s_bitcmp1_b32 %[c], 0\n"
      "s_cbranch_scc1 .Lqb0k3x%=\n"
      "v_xor_b32 %[a0], %[a0], %[w1]\n"
      "v_xor_b32 %[a1], %[a1], %[w2]\n"
      "v_xor_b32 %[a2], %[a2], %[w3]\n"
      "v_xor_b32 %[a3], %[a3], %[w4]\n"
      "v_xor_b32 %[a4], %[a4], %[w5]\n"
      "v_xor_b32 %[a5], %[a5], %[w6]\n"
      "v_xor_b32 %[a6], %[a6], %[w7]\n"
      "v_xor_b32 %[a7], %[a7], %[w8]\n"
      "v_xor_b32 %[a8], %[a8], %[w9]\n"
      "v_xor_b32 %[a9], %[a9], %[w10]\n"
      "s_branch .Lqendx%=\n"
      ".Lqb0k3x%=:\n"
      "v_bitop3_b32 %[a0], %[a0], %[w0], %[w1] bitop3:0x96\n"
      "v_bitop3_b32 %[a1], %[a1], %[w1], %[w2] bitop3:0x96\n"
      "v_bitop3_b32 %[a2], %[a2], %[w2], %[w3] bitop3:0x96\n"
      "v_bitop3_b32 %[a3], %[a3], %[w3], %[w4] bitop3:0x96\n"
      "v_bitop3_b32 %[a4], %[a4], %[w4], %[w5] bitop3:0x96\n"
      "v_bitop3_b32 %[a5], %[a5], %[w5], %[w6] bitop3:0x96\n"
      "v_bitop3_b32 %[a6], %[a6], %[w6], %[w7] bitop3:0x96\n"
      "v_bitop3_b32 %[a7], %[a7], %[w7], %[w8] bitop3:0x96\n"
      "v_bitop3_b32 %[a8], %[a8], %[w8], %[w9] bitop3:0x96\n"
      "v_bitop3_b32 %[a9], %[a9], %[w9], %[w10] bitop3:0x96\n"
      "s_branch .Lqendx%=\n"
      ".Lqb2k4x%=:\n"
      "s_bitcmp1_b32 %[c], 1\n"
      "s_cbranch_scc1 .Lqb1k6x%=\n"
      "s_bitcmp1_b32 %[c], 0\n"
      "s_cbranch_scc1 .Lqb0k5x%=\n"
      "v_xor_b32 %[a0], %[a0], %[w2]\n"
      "v_xor_b32 %[a1], %[a1], %[w3]\n"
      "v_xor_b32 %[a2], %[a2], %[w4]\n"
      "v_xor_b32 %[a3], %[a3], %[w5]\n"
      "v_xor_b32 %[a4], %[a4], %[w6]\n"
      "v_xor_b32 %[a5], %[a5], %[w7]\n"
      "v_xor_b32 %[a6], %[a6], %[w8]\n"
      "v_xor_b32 %[a7], %[a7], %[w9]\n"
      "v_xor_b32 %[a8], %[a8], %[w10]\n"
      "v_xor_b32 %[a9], %[a9], %[w11]\n"
      "s_branch .Lqendx%=\n"
      ".Lqb0k5x%=:\n"
      "v_bitop3_b32 %[a0], %[a0], %[w0], %[w2] bitop3:0x96\n"
      "v_bitop3_b32 %[a1], %[a1], %[w1], %[w3] bitop3:0x96\n"
      "v_bitop3_b32 %[a2], %[a2], %[w2], %[w4] bitop3:0x96\n"
      "v_bitop3_b32 %[a3], %[a3], %[w3], %[w5] bitop3:0x96\n"
      "v_bitop3_b32 %[a4], %[a4], %[w4], %[w6] bitop3:0x96\n"
      "v_bitop3_b32 %[a5], %[a5], %[w5], %[w7] bitop3:0x96\n"
      "v_bitop3_b32 %[a6], %[a6], %[w6], %[w8] bitop3:0x96\n"
      "v_bitop3_b32 %[a7], %[a7], %[w7], %[w9] bitop3:0x96\n"
      "v_bitop3_b32 %[a8], %[a8], %[w8], %[w10] bitop3:0x96\n"
      "v_bitop3_b32 %[a9], %[a9], %[w9], %[w11] bitop3:0x96\n"
      "s_branch .Lqendx%=\n"
      ".Lqb1k6x%=:\n"
      "s_bitcmp1_b32 %[c], 0\n"
      "s_cbranch_scc1 .Lqb0k7x%=\n"
      "v_bitop3_b32 %[a0], %[a0], %[w1], %[w2] bitop3:0x96\n"
      "v_bitop3_b32 %[a1], %[a1], %[w2], %[w3] bitop3:0x96\n"
      "v_bitop3_b32 %[a2], %[a2], %[w3], %[w4] bitop3:0x96\n"
      "v_bitop3_b32 %[a3], %[a3], %[w4], %[w5] bitop3:0x96\n"
      "v_bitop3_b32 %[a4], %[a4], %[w5], %[w6] bitop3:0x96\n"
      "v_bitop3_b32 %[a5], %[a5], %[w6], %[w7] bitop3:0x96\n"
      "v_bitop3_b32 %[a6], %[a6], %[w7], %[w8] bitop3:0x96\n"
      "v_bitop3_b32 %[a7], %[a7], %[w8], %[w9] bitop3:0x96\n"
      "v_bitop3_b32 %[a8], %[a8], %[w9], %[w10] bitop3:0x96\n"
      "v_bitop3_b32 %[a9], %[a9], %[w10], %[w11] bitop3:0x96\n"
      "s_branch .Lqendx%=\n"
      ".Lqb0k7x%=:\n"
      "v_bitop3_b32 %[a0], %[a0], %[w0], %[w1] bitop3:0x96\n"
      "v_xor_b32 %[a0], %[a0], %[w2]\n"
      "v_bitop3_b32 %[a1], %[a1], %[w1], %[w2] bitop3:0x96\n"
      "v_xor_b32 %[a1], %[a1], %[w3]\n"
      "v_bitop3_b32 %[a2], %[a2], %[w2], %[w3] bitop3:0x96\n"
      "v_xor_b32 %[a2], %[a2], %[w4]\n"
      "v_bitop3_b32 %[a3], %[a3], %[w3], %[w4] bitop3:0x96\n"
      "v_xor_b32 %[a3], %[a3], %[w5]\n"
      "v_bitop3_b32 %[a4], %[a4], %[w4], %[w5] bitop3:0x96\n"
      "v_xor_b32 %[a4], %[a4], %[w6]\n"
      "v_bitop3_b32 %[a5], %[a5], %[w5], %[w6] bitop3:0x96\n"
      "v_xor_b32 %[a5], %[a5], %[w7]\n"
      "v_bitop3_b32 %[a6], %[a6], %[w6], %[w7] bitop3:0x96\n"
      "v_xor_b32 %[a6], %[a6], %[w8]\n"
      "v_bitop3_b32 %[a7], %[a7], %[w7], %[w8] bitop3:0x96\n"
      "v_xor_b32 %[a7], %[a7], %[w9]\n"
      "v_bitop3_b32 %[a8], %[a8], %[w8], %[w9] bitop3:0x96\n"
      "v_xor_b32 %[a8], %[a8], %[w10]\n"
      "v_bitop3_b32 %[a9], %[a9], %[w9], %[w10] bitop3:0x96\n"
      "v_xor_b32 %[a9], %[a9], %[w11]\n"
      "s_branch .Lqendx%=\n"
      ".Lqb3k8x%=:\n"
      "s_bitcmp1_b32 %[c], 2\n"
      "s_cbranch_scc1 .Lqb2k12x%=\n"
      "s_bitcmp1_b32 %[c], 1\n"
      "s_cbranch_scc1 .Lqb1k10x%=\n"
      "s_bitcmp1_b32 %[c], 0\n"
      "s_cbranch_scc1 .Lqb0k9x%=\n"
      "v_xor_b32 %[a0], %[a0], %[w3]\n"
      "v_xor_b32 %[a1], %[a1], %[w4]\n"
      "v_xor_b32 %[a2], %[a2], %[w5]\n"
      "v_xor_b32 %[a3], %[a3], %[w6]\n"
      "v_xor_b32 %[a4], %[a4], %[w7]\n"
      "v_xor_b32 %[a5], %[a5], %[w8]\n"
      "v_xor_b32 %[a6], %[a6], %[w9]\n"
      "v_xor_b32 %[a7], %[a7], %[w10]\n"
      "v_xor_b32 %[a8], %[a8], %[w11]\n"
      "v_xor_b32 %[a9], %[a9], %[w12]\n"
      "s_branch .Lqendx%=\n"
      ".Lqb0k9x%=:\n"
      "v_bitop3_b32 %[a0], %[a0], %[w0], %[w3] bitop3:0x96\n"
      "v_bitop3_b32 %[a1], %[a1], %[w1], %[w4] bitop3:0x96\n"
      "v_bitop3_b32 %[a2], %[a2], %[w2], %[w5] bitop3:0x96\n"
      "v_bitop3_b32 %[a3], %[a3], %[w3], %[w6] bitop3:0x96\n"
      "v_bitop3_b32 %[a4], %[a4], %[w4], %[w7] bitop3:0x96\n"
      "v_bitop3_b32 %[a5], %[a5], %[w5], %[w8] bitop3:0x96\n"
      "v_bitop3_b32 %[a6], %[a6], %[w6], %[w9] bitop3:0x96\n"
      "v_bitop3_b32 %[a7], %[a7], %[w7], %[w10] bitop3:0x96\n"
      "v_bitop3_b32 %[a8], %[a8], %[w8], %[w11] bitop3:0x96\n"
      "v_bitop3_b32 %[a9], %[a9], %[w9], %[w12] bitop3:0x96\n"
      "s_branch .Lqendx%=\n"
      ".Lqb1k10x%=:\n"
      "s_bitcmp1_b32 %[c], 0\n"
      "s_cbranch_scc1 .Lqb0k11x%=\n"
      "v_bitop3_b32 %[a0], %[a0], %[w1], %[w3] bitop3:0x96\n"
      "v_bitop3_b32 %[a1], %[a1], %[w2], %[w4] bitop3:0x96\n"
      "v_bitop3_b32 %[a2], %[a2], %[w3], %[w5] bitop3:0x96\n"
      "v_bitop3_b32 %[a3], %[a3], %[w4], %[w6] bitop3:0x96\n"
      "v_bitop3_b32 %[a4], %[a4], %[w5], %[w7] bitop3:0x96\n"
      "v_bitop3_b32 %[a5], %[a5], %[w6], %[w8] bitop3:0x96\n"
      "v_bitop3_b32 %[a6], %[a6], %[w7], %[w9] bitop3:0x96\n"
      "v_bitop3_b32 %[a7], %[a7], %[w8], %[w10] bitop3:0x96\n"
      "v_bitop3_b32 %[a8], %[a8], %[w9], %[w11] bitop3:0x96\n"
      "v_bitop3_b32 %[a9], %[a9], %[w10], %[w12] bitop3:0x96\n"
      "s_branch .Lqendx%=\n"
      ".Lqb0k11x%=:\n"
      "v_bitop3_b32 %[a0], %[a0], %[w0], %[w1] bitop3:0x96\n"
      "v_xor_b32 %[a0], %[a0], %[w3]\n"
      "v_bitop3_b32 %[a1], %[a1], %[w1], %[w2] bitop3:0x96\n"
      "v_xor_b32 %[a1], %[a1], %[w4]\n"
      "v_bitop3_b32 %[a2], %[a2], %[w2], %[w3] bitop3:0x96\n"
      "v_xor_b32 %[a2], %[a2], %[w5]\n"
      "v_bitop3_b32 %[a3], %[a3], %[w3], %[w4] bitop3:0x96\n"
      "v_xor_b32 %[a3], %[a3], %[w6]\n"
      "v_bitop3_b32 %[a4], %[a4], %[w4], %[w5] bitop3:0x96\n"
      "v_xor_b32 %[a4], %[a4], %[w7]\n"
      "v_bitop3_b32 %[a5], %[a5], %[w5], %[w6] bitop3:0x96\n"
      "v_xor_b32 %[a5], %[a5], %[w8]\n"
      "v_bitop3_b32 %[a6], %[a6], %[w6], %[w7] bitop3:0x96\n"
      "v_xor_b32 %[a6], %[a6], %[w9]\n"
      "v_bitop3_b32 %[a7], %[a7], %[w7], %[w8] bitop3:0x96\n"
      "v_xor_b32 %[a7], %[a7], %[w10]\n"
      "v_bitop3_b32 %[a8], %[a8], %[w8], %[w9] bitop3:0x96\n"
      "v_xor_b32 %[a8], %[a8], %[w11]\n"
      "v_bitop3_b32 %[a9], %[a9], %[w9], %[w10] bitop3:0x96\n"
      "v_xor_b32 %[a9], %[a9], %[w12]\n"
      "s_branch .Lqendx%=\n"
      ".Lqb2k12x%=:\n"
      "s_bitcmp1_b32 %[c], 1\n"
      "s_cbranch_scc1 .Lqb1k14x%=\n"
      "s_bitcmp1_b32 %[c], 0\n"
      "s_cbranch_scc1 .Lqb0k13x%=\n"
      "v_bitop3_b32 %[a0], %[a0], %[w2], %[w3] bitop3:0x96\n"
      "v_bitop3_b32 %[a1], %[a1], %[w3], %[w4] bitop3:0x96\n"
      "v_bitop3_b32 %[a2], %[a2], %[w4], %[w5] bitop3:0x96\n"
      "v_bitop3_b32 %[a3], %[a3], %[w5], %[w6] bitop3:0x96\n"
      "v_bitop3_b32 %[a4], %[a4], %[w6], %[w7] bitop3:0x96\n"
      "v_bitop3_b32 %[a5], %[a5], %[w7], %[w8] bitop3:0x96\n"
      "v_bitop3_b32 %[a6], %[a6], %[w8], %[w9] bitop3:0x96\n"
      "v_bitop3_b32 %[a7], %[a7], %[w9], %[w10] bitop3:0x96\n"
      "v_bitop3_b32 %[a8], %[a8], %[w10], %[w11] bitop3:0x96\n"
      "v_bitop3_b32 %[a9], %[a9], %[w11], %[w12] bitop3:0x96\n"
      "s_branch .Lqendx%=\n"
      ".Lqb0k13x%=:\n"
      "v_bitop3_b32 %[a0], %[a0], %[w0], %[w2] bitop3:0x96\n"
      "v_xor_b32 %[a0], %[a0], %[w3]\n"
      "v_bitop3_b32 %[a1], %[a1], %[w1], %[w3] bitop3:0x96\n"
      "v_xor_b32 %[a1], %[a1], %[w4]\n"
      "v_bitop3_b32 %[a2], %[a2], %[w2], %[w4] bitop3:0x96\n"
      "v_xor_b32 %[a2], %[a2], %[w5]\n"
      "v_bitop3_b32 %[a3], %[a3], %[w3], %[w5] bitop3:0x96\n"
      "v_xor_b32 %[a3], %[a3], %[w6]\n"
      "v_bitop3_b32 %[a4], %[a4], %[w4], %[w6] bitop3:0x96\n"
      "v_xor_b32 %[a4], %[a4], %[w7]\n"
      "v_bitop3_b32 %[a5], %[a5], %[w5], %[w7] bitop3:0x96\n"
      "v_xor_b32 %[a5], %[a5], %[w8]\n"
      "v_bitop3_b32 %[a6], %[a6], %[w6], %[w8] bitop3:0x96\n"
      "v_xor_b32 %[a6], %[a6], %[w9]\n"
      "v_bitop3_b32 %[a7], %[a7], %[w7], %[w9] bitop3:0x96\n"
      "v_xor_b32 %[a7], %[a7], %[w10]\n"
      "v_bitop3_b32 %[a8], %[a8], %[w8], %[w10] bitop3:0x96\n"
      "v_xor_b32 %[a8], %[a8], %[w11]\n"
      "v_bitop3_b32 %[a9], %[a9], %[w9], %[w11] bitop3:0x96\n"
      "v_xor_b32 %[a9], %[a9], %[w12]\n"
      "s_branch .Lqendx%=\n"
      ".Lqb1k14x%=:\n"
      "s_bitcmp1_b32 %[c], 0\n"
      "s_cbranch_scc1 .Lqb0k15x%=\n"
      "v_bitop3_b32 %[a0], %[a0], %[w1], %[w2] bitop3:0x96\n"
      "v_xor_b32 %[a0], %[a0], %[w3]\n"
      "v_bitop3_b32 %[a1], %[a1], %[w2], %[w3] bitop3:0x96\n"
      "v_xor_b32 %[a1], %[a1], %[w4]\n"
      "v_bitop3_b32 %[a2], %[a2], %[w3], %[w4] bitop3:0x96\n"
      "v_xor_b32 %[a2], %[a2], %[w5]\n"
      "v_bitop3_b32 %[a3], %[a3], %[w4], %[w5] bitop3:0x96\n"
      "v_xor_b32 %[a3], %[a3], %[w6]\n"
      "v_bitop3_b32 %[a4], %[a4], %[w5], %[w6] bitop3:0x96\n"
      "v_xor_b32 %[a4], %[a4], %[w7]\n"
      "v_bitop3_b32 %[a5], %[a5], %[w6], %[w7] bitop3:0x96\n"
      "v_xor_b32 %[a5], %[a5], %[w8]\n"
      "v_bitop3_b32 %[a6], %[a6], %[w7], %[w8] bitop3:0x96\n"
      "v_xor_b32 %[a6], %[a6], %[w9]\n"
      "v_bitop3_b32 %[a7], %[a7], %[w8], %[w9] bitop3:0x96\n"
      "v_xor_b32 %[a7], %[a7], %[w10]\n"
      "v_bitop3_b32 %[a8], %[a8], %[w9], %[w10] bitop3:0x96\n"
      "v_xor_b32 %[a8], %[a8], %[w11]\n"
      "v_bitop3_b32 %[a9], %[a9], %[w10], %[w11] bitop3:0x96\n"
      "v_xor_b32 %[a9], %[a9], %[w12]\n"
      "s_branch .Lqendx%=\n"
      ".Lqb0k15x%=:\n"
      "v_bitop3_b32 %[a0], %[a0], %[w0], %[w1] bitop3:0x96\n"
      "v_bitop3_b32 %[a0], %[a0], %[w2], %[w3] bitop3:0x96\n"
      "v_bitop3_b32 %[a1], %[a1], %[w1], %[w2] bitop3:0x96\n"
      "v_bitop3_b32 %[a1], %[a1], %[w3], %[w4] bitop3:0x96\n"
      "v_bitop3_b32 %[a2], %[a2], %[w2], %[w3] bitop3:0x96\n"
      "v_bitop3_b32 %[a2], %[a2], %[w4], %[w5] bitop3:0x96\n"
      "v_bitop3_b32 %[a3], %[a3], %[w3], %[w4] bitop3:0x96\n"
      "v_bitop3_b32 %[a3], %[a3], %[w5], %[w6] bitop3:0x96\n"
      "v_bitop3_b32 %[a4], %[a4], %[w4], %[w5] bitop3:0x96\n"
      "v_bitop3_b32 %[a4], %[a4], %[w6], %[w7] bitop3:0x96\n"
      "v_bitop3_b32 %[a5], %[a5], %[w5], %[w6] bitop3:0x96\n"
      "v_bitop3_b32 %[a5], %[a5], %[w7], %[w8] bitop3:0x96\n"
      "v_bitop3_b32 %[a6], %[a6], %[w6], %[w7] bitop3:0x96\n"
      "v_bitop3_b32 %[a6], %[a6], %[w8], %[w9] bitop3:0x96\n"
      "v_bitop3_b32 %[a7], %[a7], %[w7], %[w8] bitop3:0x96\n"
      "v_bitop3_b32 %[a7], %[a7], %[w9], %[w10] bitop3:0x96\n"
      "v_bitop3_b32 %[a8], %[a8], %[w8], %[w9] bitop3:0x96\n"
      "v_bitop3_b32 %[a8], %[a8], %[w10], %[w11] bitop3:0x96\n"
      "v_bitop3_b32 %[a9], %[a9], %[w9], %[w10] bitop3:0x96\n"
      "v_bitop3_b32 %[a9], %[a9], %[w11], %[w12] bitop3:0x96\n"
      ".Lqendx%=:\n"
      : [a0] "+v"(acc[0]), [a1] "+v"(acc[1]), [a2] "+v"(acc[2]), [a3] "+v"(acc[3]), [a4] "+v"(acc[4]), [a5] "+v"(acc[5]), [a6] "+v"(acc[6]), [a7] "+v"(acc[7]), [a8] "+v"(acc[8]), [a9] "+v"(acc[9])
      : [w0] "v"(w[0]), [w1] "v"(w[1]), [w2] "v"(w[2]), [w3] "v"(w[3]), [w4] "v"(w[4]), [w5] "v"(w[5]), [w6] "v"(w[6]), [w7] "v"(w[7]), [w8] "v"(w[8]), [w9] "v"(w[9]), [w10] "v"(w[10]), [w11] "v"(w[11]), [w12] "v"(w[12]), [c] "s"(code)
      : "scc");
}
__device__ __forceinline__ uint4 lds_b64x2(const uint32_t* p) {  // 8-byte aligned: two ds_read_b64
  const uint2 lo = *reinterpret_cast<const uint2*>(p), hi = *reinterpret_cast<const uint2*>(p + 2);
  return make_uint4(lo.x, lo.y, hi.x, hi.y);
}

// The sweep in two phases of 156 coefficient words (9984 coefficients) each, so that LDS
// holds only the x words one phase's windows read (10,624 words, 42.5 KB, plus the 624
// seeding words) instead of all 20,561: two workgroups per CU instead of one, 8 waves per
// SIMD to hide the scalar branches of the 4-bit steps.  The phases take turns in LDS
// between a wave's jobs (A B, B A, ...): the accumulation is an xor, so their order does
// not matter, and each switch regenerates the other phase's words from 624 saved ones.
constexpr int kJumpPhaseWd = 156;                     // coefficient words (of 312) per phase
constexpr int kJumpPhaseX = 64 * kJumpPhaseWd + 640;  // x words a phase reads: 9984 + 10 x 62 + 19 + 1, rounded up
constexpr int kJumpInitOff = kJumpXOff + kJumpPhaseX;  // the 624 seeding words, kept for phase A
constexpr int kJumpLds2Words = kJumpInitOff + kMtN;

__global__ __launch_bounds__(kJumpThreads) void fks_jump_kernel(JumpArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_j[];
  uint32_t* lx = lds_j + kJumpXOff;  // phase P: lx[t] = x[9984 P + t]
  uint32_t* x0 = lds_j + kJumpInitOff;
  const int tid = threadIdx.x;
  const int k = blockIdx.x;
  const uint64_t seed = a.seeds[k];
  // mt19937::init_with_uint32 (MT19937RNGEngine.h:156-162): a serial recurrence
  if (tid == 0) {
    uint32_t s = (uint32_t)(seed & 0xffffffffu);
    x0[0] = s;
    for (int j = 1; j < kMtN; j++) {
      s = 1812433253u * (s ^ (s >> 30)) + (uint32_t)j;
      x0[j] = s;
    }
  }
  __syncthreads();
  // fill LDS with phase P's words: its first 624 (the seeding words, or x[9984..10607]
  // from phase A's words in place), then x[n] = x[n-227] ^ twist(x[n-624], x[n-623]) in
  // steps of 227 independent words.  Callers are past a barrier that ends every read of
  // the other phase.
  auto fill = [&](const int P) {
    if (tid < kMtN) lx[tid] = P == 0 ? x0[tid] : lx[64 * kJumpPhaseWd + tid];
    __syncthreads();
    for (int base = kMtN; base < kJumpPhaseX; base += kMtN - kMtM) {
      const int n = base + tid;
      if (tid < kMtN - kMtM && n < kJumpPhaseX) lx[n] = lx[n - (kMtN - kMtM)] ^ mt_twist(lx[n - kMtN], lx[n - kMtN + 1]);
      __syncthreads();
    }
  };
  fill(0);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  constexpr int kW = 10, kLanes = 63;  // 63 lanes x 10 words (lane 62 keeps words 620..623)
  const uint32_t* yb = lx + 1 + kW * lane;  // y[9984 P + kW lane]
  const int c0 = blockIdx.y * a.chunks_per_wg;
  const int c1 = min(c0 + a.chunks_per_wg, a.nchunks);
  const int st = a.stride > 0 ? a.stride : 1;
  constexpr int kWaves = kJumpThreads / 64;
  const int nround = (c1 - c0 + kWaves - 1) / kWaves;  // workgroup-uniform
  int P = 0;  // the phase in LDS
  for (int r = 0; r < nround; r++) {
    const int c = c0 + wave + kWaves * r;
    const bool job = c < c1 && lane < kLanes;
    const int64_t b = c < c1 ? a.chunk_block[(size_t)c * st] : 0;
    const bool sweep = c < c1 && b != 0;  // wave-uniform
    const uint64_t* poly = a.polys + (size_t)(c < c1 ? c : c0) * st * 312;  // wave-uniform: scalar loads
    uint32_t acc[kW];
#pragma unroll
    for (int j = 0; j < kW; j++) acc[j] = 0u;
    if (job && b == 0) {
#pragma unroll
      for (int j = 0; j < kW; j++) acc[j] = kW * lane + j < kMtN ? x0[kW * lane + j] : 0u;
    }
    for (int h = 0; h < 2; h++) {
      if (h == 1) {  // switch the phase in LDS
        __syncthreads();
        P ^= 1;
        fill(P);
      }
      if (sweep && lane < kLanes) {
        uint32_t win[16];
        {
          const uint4 q0 = lds_b64x2(yb), q1 = lds_b64x2(yb + 4), q2 = lds_b64x2(yb + 8), q3 = lds_b64x2(yb + 12);
          win[0] = q0.x; win[1] = q0.y; win[2] = q0.z; win[3] = q0.w;
          win[4] = q1.x; win[5] = q1.y; win[6] = q1.z; win[7] = q1.w;
          win[8] = q2.x; win[9] = q2.y; win[10] = q2.z; win[11] = q2.w;
          win[12] = q3.x; win[13] = q3.y; win[14] = q3.z; win[15] = q3.w;
        }
        const uint64_t* pw = poly + kJumpPhaseWd * P;
        uint64_t next = pw[0];
        for (int wd = 0; wd < kJumpPhaseWd; wd++) {
          const uint64_t bits = next;
          if (wd + 1 < kJumpPhaseWd) next = pw[wd + 1];  // prefetch the next 64 coefficients
          const uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
          const uint32_t* yw = yb + 64 * wd;
#pragma unroll
          for (int q = 0; q < 16; q++) {
            // window = y[9984 P + 64 wd + 4q + kW lane + 0..15], stored rotated by 4q (mod 16)
            const uint4 nx = lds_b64x2(yw + 4 * q + 16);
            const int rot = (4 * q) & 15;
            const uint32_t word = q < 8 ? lo : hi;
            const uint32_t quad = (word >> ((4 * q) & 31)) & 15u;
            uint32_t w13[13];
#pragma unroll
            for (int t = 0; t < 13; t++) w13[t] = win[(rot + t) & 15];
            jump_quad_step10(acc, w13, quad);
            win[(rot + 0) & 15] = nx.x;
            win[(rot + 1) & 15] = nx.y;
            win[(rot + 2) & 15] = nx.z;
            win[(rot + 3) & 15] = nx.w;
          }
        }
      }
    }
    if (job) {
      uint32_t* out = a.states + ((size_t)(a.use_slot ? a.slot[k] : (uint32_t)k) * a.nchunks + c) * kMtN + kW * lane;
#pragma unroll
      for (int j = 0; j < kW; j += 2)
        if (kW * lane + j < kMtN) *reinterpret_cast<uint2*>(out + j) = make_uint2(acc[j], acc[j + 1]);
    }
  }
}

}  // namespace
}  // namespace fks
