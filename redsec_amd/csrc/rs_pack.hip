// rs_pack.hip -- packed results (rs_pack_dev; include/redsec_hip.h): LWE samples keyswitched into the coefficients of RLWE ciphertexts
//   pack_init_kernel   rlwe[r] = (0, sum_c b_(rN+c) X^c)
//   pack_kernel        rlwe[r] -= sum over a chunk of (i, j) of D_ij(X) K[i][j],  D_ij(X) = sum_c digit_j(abar_i of sample rN + c) X^c
// An object of its own, so that every earlier kernel keeps its instructions. Integer only: a basebit-bit digit times a 32-bit word,
// accumulated mod 2^32, exact in any order, so neither the tiling nor the number of chunks can change a word.
//
// The shape is rlwe_pk_encrypt_kernel's (rs_rlwe.hip) with the one binary selector replaced by n t digit polynomials, each with a key
// row of its own. A workgroup of kPaThreads threads owns kPaTile consecutive coefficients of one polynomial of one ciphertext, a block
// of at most kPaSlots slots c0 .. c0 + cn - 1 and a chunk of kPaSeg = 8 LWE indices (rs_pack.h: one ciphertext alone has only
// 2 N / 512 tiles, with the chunks default-128 has 316 workgroups per ciphertext). Per key row (i, j) it stages the window of
// ext = (-p, p) its coefficients and slots read, cpad + kPaTile words with cpad = cn rounded up to 4, so that ten slots stage and sweep
// ten slots, not N, and runs the sweep of rs_ring_sweep.h (the LDS read pattern, the scalar digit and the multiply-add form are
// described there) with pa_digit; thread t keeps its four coefficients in registers over all its rows. What is this kernel's own:
// the sample words of the chunk, kPaSeg consecutive i per sample (32 contiguous bytes), are read once and transposed through LDS
// into s_a[ii][c] = a_i + offset, zero in the padding, so that the sweep over c reads them as its 16-byte broadcast per four slots
// and never walks a column of ct at stride n + 1; and the loop over the key rows, each staged between two barriers.
// THE SWEEP IS WRITTEN OUT HERE, not a call of ring_sweep: with the call this kernel compiled to the same instruction mix in
// another order and measured 8.2 % slower at 1,024 slots and 3.1 % at 65,536 (profiles/r29/, same box, three runs a side), where
// ring_rekey_kernel and ring_cmux_kernel kept their times. So this is the ONE copy of ring_sweep left: a change to the loop in
// rs_ring_sweep.h has to be made below too. rs_emu_pack (rs_emulate.cpp) walks the same workgroups and rows on the CPU and does
// call ring_sweep, so tests/test_pack_cpu.py pins the shared loop and the placement, not the lines below.
// The partial sums of the slot blocks and index chunks meet by vector atomicAdd (global_atomic_add_u32, no return) on the words that
// pack_init_kernel has set on the same stream just before; every call initialises again, so a second call into the same buffer gives
// the same words.
// Resources (-Rpass-analysis=kernel-resource-usage): pack_kernel 35 VGPRs, 48 SGPRs, (9 cpad + 512) 4 bytes of dynamic LDS (2.5 KB at
// ten slots, 38.0 KB at 1,024), no scratch, no static LDS, eight waves per SIMD by registers (four workgroups per CU by LDS at full
// slot blocks); pack_init_kernel 13 VGPRs, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include "rs_kernels.h"
#include "rs_pack.h"

namespace rs {

__global__ __launch_bounds__(kPaInitThreads) void pack_init_kernel(PackArgs a, long words) {
  const long idx = (long)blockIdx.x * kPaInitThreads + threadIdx.x;
  if (idx >= words) return;
  const int N = a.N;
  const long r = idx / (2 * (long)N);
  const int w = (int)(idx - r * 2 * (long)N);
  uint32_t v = 0u;
  if (w >= N) {
    const long s = r * (long)N + (w - N);
    if (s < a.count) v = (uint32_t)a.ct[(size_t)s * ((size_t)a.n + 1) + (size_t)a.n];
  }
  a.rlwe[idx] = (int32_t)v;
}

__global__ __launch_bounds__(kPaThreads) void pack_kernel(PackArgs a, int chunks, int slot_blocks) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_lds[];
  const int N = a.N, n = a.n, tiles = N / kPaTile, t = threadIdx.x;
  unsigned g = blockIdx.x;
  const int tile = (int)(g % (unsigned)tiles); g /= (unsigned)tiles;
  const int poly = (int)(g & 1u); g >>= 1;
  const int sb = (int)(g % (unsigned)slot_blocks); g /= (unsigned)slot_blocks;
  const int chunk = (int)(g % (unsigned)chunks);
  const long r = (long)(g / (unsigned)chunks);
  const int c0 = sb * kPaSlots, slots = pa_slots(a.count, N, r);
  if (c0 >= slots) return;                                  // the whole workgroup: this ciphertext has no slot in the block
  const int cn = slots - c0 < kPaSlots ? slots - c0 : kPaSlots, cpad = pa_pad4(cn);
  uint32_t* s_win = s_lds;                                  // [cpad + kPaTile]: ext[wb + x]
  uint32_t* s_a = s_lds + cpad + kPaTile;                   // [kPaSeg][cpad]: a_i + offset of slot c0 + cc, 0 in the padding
  const int i0 = chunk * kPaSeg, segn = n - i0 < kPaSeg ? n - i0 : kPaSeg;
  const int k0 = tile * kPaTile, wb = pa_window_base(N, k0, c0, cpad);
  const uint32_t off = pa_offset(a.basebit, a.t), mask = (1u << a.basebit) - 1u;
  const uint32_t* ct = reinterpret_cast<const uint32_t*>(a.ct) + ((size_t)r * (size_t)N + (size_t)c0) * ((size_t)n + 1);
  const uint32_t* key = reinterpret_cast<const uint32_t*>(a.key);
  const uint4* win4 = reinterpret_cast<const uint4*>(s_win);
  uint32_t acc[kPaKpt] = {0u, 0u, 0u, 0u};
  for (int idx = t; idx < segn * cpad; idx += kPaThreads) {
    const int cc = idx / segn, ii = idx - cc * segn;        // consecutive threads: consecutive words of one sample
    s_a[ii * cpad + cc] = cc < cn ? ct[(size_t)cc * ((size_t)n + 1) + (size_t)(i0 + ii)] + off : 0u;
  }
  for (int ii = 0; ii < segn; ++ii) {
    const uint4* a4 = reinterpret_cast<const uint4*>(s_a + ii * cpad);
    for (int j = 0; j < a.t; ++j) {
      const uint32_t* p = key + pa_key_offset(N, a.t, i0 + ii, j, poly);
      __syncthreads();                                    // the previous row's sweep has read the window
      for (int x = t; x < cpad + kPaTile; x += kPaThreads) s_win[x] = rl_ext_word(p, N, wb + x);
      __syncthreads();
      // ring_sweep(s_win, s_a + ii * cpad, cpad, t, pa_digit(., basebit, j), acc), written out (see the header comment)
      const int shift = 32 - (j + 1) * a.basebit;
      int c4 = t + cpad / 4;                              // chunk of window words 4t + cpad - cc .. + 3, cc = 0
      uint4 hi = win4[c4];
      for (int q4 = 0; q4 < cpad / 4; ++q4) {             // slots cc = 4 q4 .. 4 q4 + 3
        const uint4 av = a4[q4];                          // the same four words in every lane: scalars
        const uint32_t d[4] = {((uint32_t)__builtin_amdgcn_readfirstlane((int)av.x) >> shift) & mask,
                               ((uint32_t)__builtin_amdgcn_readfirstlane((int)av.y) >> shift) & mask,
                               ((uint32_t)__builtin_amdgcn_readfirstlane((int)av.z) >> shift) & mask,
                               ((uint32_t)__builtin_amdgcn_readfirstlane((int)av.w) >> shift) & mask};
        const uint4 lo = win4[--c4];
        const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int b = 0; b < 4; ++b) {                     // slot cc = 4 q4 + b: coefficient 4t + q takes window word 4 c4' + q - b
#pragma unroll
          for (int q = 0; q < kPaKpt; ++q) acc[q] += w[4 + q - b] * d[b];
        }
        hi = lo;
      }
    }
  }
  unsigned int* out = reinterpret_cast<unsigned int*>(a.rlwe) + ((size_t)r * 2 + (size_t)poly) * (size_t)N + k0 + kPaKpt * t;
#pragma unroll
  for (int q = 0; q < kPaKpt; ++q) atomicAdd(out + q, 0u - acc[q]);
}

hipError_t launch_pack(const PackArgs& a, hipStream_t st) {
  if (a.count <= 0) return hipSuccess;
  const long R = (a.count + a.N - 1) / a.N, words = R * 2 * (long)a.N;
  const int sbs = pa_slot_blocks(a.count, a.N), chunks = pa_chunks(a.n);
  hipLaunchKernelGGL(pack_init_kernel, dim3((unsigned)((words + kPaInitThreads - 1) / kPaInitThreads)), dim3(kPaInitThreads), 0, st, a, words);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const long full = a.count < a.N ? a.count : (long)a.N;
  const int cpad = pa_pad4((int)(full < kPaSlots ? full : (long)kPaSlots));
  const size_t lds = ((size_t)cpad * (1 + kPaSeg) + kPaTile) * sizeof(uint32_t);
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)pa_groups(a.count, a.n, a.N)), dim3(kPaThreads), lds, st, a, chunks, sbs);
  return hipGetLastError();
}

}  // namespace rs
