// LFT horizon sweep for small augmented dimension (s <= 5): one problem per
// LANE.  At s = 5 a 16-lane row per problem (lft_sweep.hip) leaves 11 of 16
// lanes idle and runs 4 problems per wave-instruction; here every lane owns
// one problem, all its s x s blocks live in registers, and a wave-instruction
// advances 64 problems.  Same algorithm, _sym placement, chol_inv jitter ladder
// and status bits as horizon_selection.py:36-86 / utils.py:69-93.
//
// Streaming: step k+1's Q, A, B (and, after the query, QT) blocks of the
// wave's 64 problems are loaded into LDS by LDS-DMA while step k computes.
// Pieces are chunk-major: piece r holds the r-th 16-byte chunk of every lane's
// block, so a lane reads its own chunk at base + 1024 r + 16 lane (conflict-free
// ds_read_b128) and the DMA source of lane l is simply block(l) + 16 r.
#include <stdlib.h>

#include "hop_device.hpp"
#include "hop_kernels.hpp"


namespace hop {
namespace small {
// 1/d as v_rcp + one Newton step (the IEEE division sequence is ~10 instructions)
__device__ __forceinline__ float small_recip(float d) {
  const float r = __builtin_amdgcn_rcpf(d);
  return __builtin_fmaf(r, __builtin_fmaf(-d, r, 1.0f), r);
}
__device__ __forceinline__ double small_recip(double d) {
  const double r = __builtin_amdgcn_rcp(d);
  return __builtin_fma(r, __builtin_fma(-d, r, 1.0), r);
}
}  // namespace small
}  // namespace hop

#include "small_math.hpp"

namespace hop {
namespace small {

// fp32 blocks (config 3's tile64 path): the query eliminates Sigma_eps + X_t directly
// (round 3's cond_query_direct).  The congruence form exists for the augmented
// terminal block's rho_reg = 1e-12 (sigma ~ 1e-9), which fp32 blocks cannot carry
// anyway; on fp32 it only cost config 3 1.8 %.  The
// fp64 kernels and the trajectory form keep the congruence query.
#ifndef HOP_SMALL_F32_DIRECT
#define HOP_SMALL_F32_DIRECT 1
#endif
constexpr bool kSmallF32Direct = HOP_SMALL_F32_DIRECT != 0;

// One 16-B chunk per lane into LDS.  The blocks are read exactly once, so the
// stream is non-temporal (nt): config 3 (B = 65536, N = 200, fp32 tile64) takes
// 0.777 ms against 0.873 ms with the default policy (tools/ab_libs.py, same
// process), bitwise equal; sc1 alone changes nothing.
__device__ __forceinline__ void dma16(unsigned voff, __amdgpu_buffer_rsrc_t rsrc, unsigned lds,
                                      unsigned soff) {
  unsigned keep;
  asm volatile(
      HOP_VMNOP  // (hop_device.hpp)
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %1, %2, %4 offen nt lds\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(rsrc), "s"(__builtin_amdgcn_readfirstlane(lds)),
        "s"(__builtin_amdgcn_readfirstlane(soff))
      : "memory");
}

// Tile64 blocks: the pieces of a block are contiguous 1-KiB spans in HBM and in LDS,
// and the LDS-DMA instruction offset is added to both addresses (measured,
// tools/ubench/lds_dma_offset.hip), so up to four pieces share one M0 and one
// voffset: group g loads pieces 4g .. 4g+3 at M0 = block + 4096 g, offsets 0 .. 3072.
// Five instructions per group instead of five per piece.
template <int NL>
__device__ __forceinline__ void dma_grp(unsigned voff, __amdgpu_buffer_rsrc_t rsrc, unsigned lds,
                                        unsigned soff) {
  static_assert(NL >= 1 && NL <= 4, "one to four pieces per M0");
  unsigned keep;
#define HOP_G(OFF) "buffer_load_dwordx4 %1, %2, %4 offen offset:" #OFF " nt lds\n\t"
  const unsigned l = __builtin_amdgcn_readfirstlane(lds), so = __builtin_amdgcn_readfirstlane(soff);
  if constexpr (NL == 1)
    asm volatile(HOP_VMNOP "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t" HOP_G(0) "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(l), "s"(so) : "memory");
  else if constexpr (NL == 2)
    asm volatile(HOP_VMNOP "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t" HOP_G(0) HOP_G(1024)
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(l), "s"(so) : "memory");
  else if constexpr (NL == 3)
    asm volatile(HOP_VMNOP "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t" HOP_G(0) HOP_G(1024)
                 HOP_G(2048) "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(l), "s"(so) : "memory");
  else
    asm volatile(HOP_VMNOP "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t" HOP_G(0) HOP_G(1024)
                 HOP_G(2048) HOP_G(3072) "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(l), "s"(so) : "memory");
#undef HOP_G
}
// NP pieces of one tile64 block at LDS `lds`, the last one LAST lanes wide (64: full);
// vr[r] = 1024 r + 16 lane (the block's per-piece voffsets)
template <int NP, int LAST>
__device__ __forceinline__ void dma_block64(const unsigned* vr, __amdgpu_buffer_rsrc_t rsrc,
                                            unsigned lds, unsigned soff, int lane) {
  constexpr int FULL = LAST == 64 ? NP : NP - 1;
  static_for<(FULL + 3) / 4>([&](auto G_) {
    constexpr int g = G_;
    constexpr int nl = FULL - 4 * g < 4 ? FULL - 4 * g : 4;
    dma_grp<nl>(vr[4 * g], rsrc, lds + 4096u * g, soff);
  });
  if constexpr (FULL < NP) {
    if (lane < LAST) dma16(vr[NP - 1], rsrc, lds + 1024u * (NP - 1), soff);
  }
}
// the same from the block's base voffset v0 (piece r at v0 + 1024 r)
template <int NP, int LAST>
__device__ __forceinline__ void dma_block64v(unsigned v0, __amdgpu_buffer_rsrc_t rsrc,
                                             unsigned lds, unsigned soff, int lane) {
  constexpr int FULL = LAST == 64 ? NP : NP - 1;
  static_for<(FULL + 3) / 4>([&](auto G_) {
    constexpr int g = G_;
    constexpr int nl = FULL - 4 * g < 4 ? FULL - 4 * g : 4;
    dma_grp<nl>(v0 + 4096u * g, rsrc, lds + 4096u * g, soff);
  });
  if constexpr (FULL < NP) {
    if (lane < LAST) dma16(v0 + 1024u * (NP - 1), rsrc, lds + 1024u * (NP - 1), soff);
  }
}

// PW problems per wave: 64 (one per lane), or 32 (lanes 32..63 recompute lanes
// 0..31's problems and store nothing) so that a batch of 64 problems per SIMD
// runs as two waves per SIMD that hide each other's dependency stalls
template <class T, int S, int MM, int PW = 64>
struct Geo {
  static constexpr int CM = (S * S * (int)sizeof(T) + 15) / 16;   // chunks per s x s block
  static constexpr int CB = (S * MM * (int)sizeof(T) + 15) / 16;  // chunks per B block
  static constexpr int P_Q = 0, P_A = CM, P_B = 2 * CM, P_T = 2 * CM + CB;
  static constexpr int PIECES = 3 * CM + CB;
  static constexpr int PIECE = 16 * PW;  // bytes per piece (one 16-B chunk per problem)
  static constexpr int WAVE_BYTES = PIECES * PIECE;
  // waves per block: 4, or as many as fit the CU's 160 KiB of LDS (fp64 s = 5: 42 KiB
  // per wave of 64 problems, 3 waves per block)
  static constexpr int WPB = (160 * 1024) / WAVE_BYTES < 4 ? (160 * 1024) / WAVE_BYTES : 4;
  static_assert(WPB >= 1, "one wave's images must fit in LDS");
  static constexpr int TPB = 64 * WPB;
  static constexpr int PPB = WPB * PW;  // problems per block
  // tile64 layout: a block's 64 problems are 64 S S (64 S MM) contiguous elements;
  // lanes loading the last piece of a section (the rest would be the next step's)
  static constexpr int LAST_M = (64 * S * S * (int)sizeof(T) - (CM - 1) * 1024) / 16;
  static constexpr int LAST_B = (64 * S * MM * (int)sizeof(T) - (CB - 1) * 1024) / 16;
};

// read an (R x C) row-major block from the wave's LDS image.  LY 0: chunk-major
// (piece r = the r-th 16-B chunk of every problem), LY 1: problem-major (the
// problem's CH chunks contiguous at 16 CH slot), LY 2: element-major (element e of
// problem p at TS (64 e + p): the image of the tiled HBM layout)
template <class T, int R, int C, int P0, int PIECE = 1024, int LY = 0>
__device__ __forceinline__ void read_block(const unsigned char* wimg, int slot, T (&out)[R][C]) {
  constexpr int NE = R * C, CH = (NE * (int)sizeof(T) + 15) / 16, PER = 16 / (int)sizeof(T);
  if constexpr (LY == 2) {
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < C; ++j)
        out[i][j] = *reinterpret_cast<const T*>(wimg + P0 * 1024 +
                                                 (int)sizeof(T) * (64 * (i * C + j) + slot));
    return;
  }
  T buf[CH * PER];
#pragma unroll
  for (int r = 0; r < CH; ++r) {
    const float4 v = *reinterpret_cast<const float4*>(
        LY == 1 ? wimg + P0 * 1024 + 16 * (CH * slot + r) : wimg + (P0 + r) * PIECE + 16 * slot);
    const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
    for (int q = 0; q < PER; ++q) buf[r * PER + q] = e[q];
  }
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = 0; j < C; ++j) out[i][j] = buf[i * C + j];
}

// COND: the conditioned-prefix association (small_math.hpp cond_*; DESIGN.md
// 3.0) with first-attempt inverses; problems it cannot take get status 16 and
// are recomputed by the LFT instantiation in rerun mode (a.cond & kCondRerun).
// EXP (developer builds, timing experiments only -- results are wrong): 1 drops
// the arithmetic (the LDS images are only summed), 2 streams step 0 only
// PM: problem-major pieces (the wave's 64 CM chunks of a block in problem order,
// so a wave-instruction reads ~64 / CM contiguous spans of 16 CM bytes instead of
// 64 scattered 16-B chunks); only with PW = 64
// LY 2 (timing experiment): the tiled HBM layout [B/64][nalloc][block elements][64]
template <class T, int S, int MM, bool COND = false, int PW = 64, int EXP = 0, int LY = 0>
__device__ __forceinline__ void lft_small_body(const LftArgs<T>& a) {
  using G = Geo<T, S, MM, PW>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63, slot = lane & (PW - 1);
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned char* wimg = smem_raw + w * G::WAVE_BYTES;
  const unsigned wlds = (unsigned)(uintptr_t)wimg;
  const long long wave_prob0 = (long long)blockIdx.x * G::PPB + w * PW;
  const long long prob = wave_prob0 + slot;
  const bool owner = PW == 64 || lane < PW;  // lanes past PW duplicate lane - PW
  bool valid = owner && prob < a.batch;
  const long long pb = prob < a.batch ? prob : a.batch - 1;
  if (wave_prob0 >= a.batch) return;  // wave-uniform; no workgroup barrier in this kernel
  const long long pb0 = wave_prob0;
  if (!COND && (a.cond & kCondRerun)) {  // only the problems the COND kernel handed over
    const bool need = valid && (a.status[prob] & 16);
    if (!__any(need)) return;  // wave-uniform; no workgroup barrier in this kernel
    valid = need;
  }
  const int N = a.n, mt = a.max_tries;
  constexpr int SS = S * S, SM = S * MM, TS = (int)sizeof(T);
  const long long pstrM = (long long)a.nalloc * SS * TS, pstrB = (long long)a.nalloc * SM * TS;
  auto mk = [&](const T* base, long long pstr) {
    // exact bounds: range checking is per dword (tools/ubench_oob.hip), so a chunk
    // straddling the tensor end returns its valid dwords and zeros
    // (tile64: the tile is allocated whole, padding slots included)
    const long long left = (LY == 2 ? 64 : a.batch - pb0) * pstr;
    const unsigned nrec = left > 0xFFFFFFF0ll ? 0xFFFFFFF0u : (unsigned)left;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(base) + pb0 * (pstr / TS), (short)0,
                                             (int)nrec, 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t rQ = mk(a.Q, pstrM), rA = mk(a.A, pstrM), rT = mk(a.QT, pstrM),
                               rB = mk(a.B, pstrB);
  static_assert(LY == 0 || PW == 64, "layouts 1, 2 need 64 problems per wave");
  constexpr bool PM = LY == 1;
  unsigned vMr[G::CM], vBr[G::CB];  // per-piece lane source offsets (problem part)
#pragma unroll
  for (int r = 0; r < G::CM; ++r) {
    const int q = 64 * r + lane, pp = PM ? q / G::CM : slot, cc = PM ? q % G::CM : r;
    const long long pe = wave_prob0 + pp < a.batch ? wave_prob0 + pp : a.batch - 1;
    vMr[r] = LY == 2 ? 1024u * r + 16u * lane : (unsigned)((pe - pb0) * pstrM) + 16u * cc;
  }
#pragma unroll
  for (int r = 0; r < G::CB; ++r) {
    const int q = 64 * r + lane, pp = PM ? q / G::CB : slot, cc = PM ? q % G::CB : r;
    const long long pe = wave_prob0 + pp < a.batch ? wave_prob0 + pp : a.batch - 1;
    vBr[r] = LY == 2 ? 1024u * r + 16u * lane : (unsigned)((pe - pb0) * pstrB) + 16u * cc;
  }
  // LDS-DMA writes lane l's 16 B at M0 + 16 l: with PW = 32 only the owner lanes
  // load (the duplicates would write into the next piece)
  auto dma_stage = [&](int k) {  // Q, A, B of step k
    const unsigned soM = (unsigned)(k * SS * TS * (LY == 2 ? 64 : 1)),
                   soB = (unsigned)(k * SM * TS * (LY == 2 ? 64 : 1));
    if constexpr (LY == 2) {  // grouped pieces (dma_block64)
      dma_block64<G::CM, G::LAST_M>(vMr, rQ, wlds + G::P_Q * 1024u, soM, lane);
      dma_block64<G::CM, G::LAST_M>(vMr, rA, wlds + G::P_A * 1024u, soM, lane);
      dma_block64<G::CB, G::LAST_B>(vBr, rB, wlds + G::P_B * 1024u, soB, lane);
    } else if (owner) {
#pragma unroll
      for (int r = 0; r < G::CM; ++r) dma16(vMr[r], rQ, wlds + (G::P_Q + r) * G::PIECE, soM);
#pragma unroll
      for (int r = 0; r < G::CM; ++r) dma16(vMr[r], rA, wlds + (G::P_A + r) * G::PIECE, soM);
#pragma unroll
      for (int r = 0; r < G::CB; ++r) dma16(vBr[r], rB, wlds + (G::P_B + r) * G::PIECE, soB);
    }
  };
  auto dma_query = [&](int k) {  // QT of step k
    const unsigned soM = (unsigned)(k * SS * TS * (LY == 2 ? 64 : 1));
    if constexpr (LY == 2) {
      dma_block64<G::CM, G::LAST_M>(vMr, rT, wlds + G::P_T * 1024u, soM, lane);
    } else if (owner) {
#pragma unroll
      for (int r = 0; r < G::CM; ++r) dma16(vMr[r], rT, wlds + (G::P_T + r) * G::PIECE, soM);
    }
  };
  auto vm_wait = []() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };

  T z[S];
#pragma unroll
  for (int i = 0; i < S; ++i) z[i] = a.z0[pb * a.z_bstride + i];
  State<T, S, MM> ps;
  ps.st = 0;
  ps.best = T(0);
  ps.tbest = 0;
  CondState<T, S, MM> cs;
  if constexpr (COND) {
    cond_init(cs, z);
    cs.bad = (a.cond & kCondFlagAll) != 0;
    cs.kf1 = cs.bad ? 1 : 0;
  }
  T rinv[MM][MM];
  {
    const T* Rp = a.R + pb * a.r_bstride;
    Gen<T, MM> r;
#pragma unroll
    for (int i = 0; i < MM; ++i)
#pragma unroll
      for (int j = 0; j < MM; ++j) r.a[i][j] = Rp[i * MM + j];
    Sym<T, MM> rs;
    sym_of(rs, r);
    if (!a.r_is_inv) spd_inverse(rs, mt, ps.st);
#pragma unroll
    for (int i = 0; i < MM; ++i)
#pragma unroll
      for (int j = 0; j < MM; ++j) rinv[i][j] = a.r_is_inv ? r.a[i][j] : rs.at(i, j);
  }
  if (N > 0) {
    dma_stage(0);
    dma_query(0);
  }
  // J ring: the values of 8 steps are written together, right after a DMA wait,
  // so that no vmcnt(0) ever waits on a scattered store and each lane writes
  // 32 contiguous bytes instead of 4 (write traffic: 409 MB -> ~J's 52 MB)
  constexpr int JR = 8;
  T jring[JR];
#pragma unroll
  for (int i = 0; i < JR; ++i) jring[i] = T(0);
  auto flush = [&](int k0, int cnt) {  // steps k0 .. k0+cnt-1 are jring[JR-cnt .. JR-1]
    if (valid) {
#pragma unroll
      for (int i = 0; i < JR; ++i)
        if (i >= JR - cnt) a.J[prob * N + k0 + i - (JR - cnt)] = jring[i];
    }
  };
#pragma unroll 1
  for (int k = 0; k < N; ++k) {
    vm_wait();     // this wave's LDS-DMA pieces of step k have landed
    wave_sync();   // (each wave owns its LDS image: no workgroup barrier)
    if (k >= JR && k % JR == 0) flush(k - JR, JR);
    {
      Gen<T, S> Q, A;
      T Bk[S][MM];
      read_block<T, S, S, G::P_Q, G::PIECE, LY>(wimg, slot, Q.a);
      read_block<T, S, S, G::P_A, G::PIECE, LY>(wimg, slot, A.a);
      read_block<T, S, MM, G::P_B, G::PIECE, LY>(wimg, slot, Bk);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (k + 1 < N && EXP != 2) dma_stage(k + 1);
      if constexpr (EXP == 1) {
        T acc = T(0);
#pragma unroll
        for (int i = 0; i < S; ++i) {
#pragma unroll
          for (int j = 0; j < S; ++j) acc += Q.a[i][j] + A.a[i][j];
#pragma unroll
          for (int j = 0; j < MM; ++j) acc += Bk[i][j];
        }
        ps.best += acc;
      } else if constexpr (COND) {
        Sym<T, S> E;
        sym_of(E, Q);
        cs.bad = cs.bad || !spd_inverse_once(E);
        cond_step<T, S, MM>(cs, E, A, Bk, rinv);
      } else {
        stage_compose<T, S, MM>(ps, k, Q, A, Bk, rinv, mt);
      }
    }
    Gen<T, S> QT;
    read_block<T, S, S, G::P_T, G::PIECE, LY>(wimg, slot, QT.a);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (k + 1 < N && EXP != 2) dma_query(k + 1);
    T jk;
    if constexpr (EXP == 1) {
      jk = ps.best;
#pragma unroll
      for (int i = 0; i < S; ++i)
#pragma unroll
        for (int j = 0; j < S; ++j) jk += QT.a[i][j];
    } else if constexpr (COND) {
      if constexpr (std::is_same_v<T, float> && kSmallF32Direct)
        jk = cond_query_direct<T, S, MM>(cs, QT);
      else
        jk = cond_query<T, S, MM>(cs, QT);
    }
    else jk = query<T, S, MM>(ps, QT, z, mt);
#pragma unroll
    for (int i = 0; i + 1 < JR; ++i) jring[i] = jring[i + 1];
    jring[JR - 1] = jk;
    if constexpr (COND) {
      take(cs, k + 1, jk, a.t_min, a.t_max);
      cond_mark(cs, k);
    } else {
      take(ps, k + 1, jk, a.t_min, a.t_max);
    }
  }
  vm_wait();
  if (N > 0) {
    const int tail = N % JR == 0 ? JR : N % JR;  // steps not flushed by the loop
    flush(N - tail, tail);
  }
  if (valid) {
    if constexpr (COND) {
      a.status[prob] = cond_status_word(cs);
      if (a.t_max > 0 && a.t_star != nullptr) {
        a.t_star[prob] = cs.tbest;
        a.j_star[prob] = cs.best;
      }
    } else {
      a.status[prob] = (int)ps.st;
      if (a.t_max > 0 && a.t_star != nullptr) {
        a.t_star[prob] = ps.tbest;
        a.j_star[prob] = ps.best;
      }
    }
  }
}

template <class T, int S, int MM, bool COND = false, int PW = 64, int EXP = 0, int LY = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PW == 64 ? 1 : 2))) void lft_small_kernel(LftArgs<T> a) {
  lft_small_body<T, S, MM, COND, PW, EXP, LY>(a);
}

// ---------------------------------------------------------------------------
// The pipelined rerun for s <= 5 (fp64 augmented blocks).  The
// rerun launch used to recompute every hand-over on its own lane from k = 0: the
// whole step on one lane, ~12 us per step when the blocks reach chol_inv's ladder
// (the point-mass obstacle cost: every select hands over).  Only the prefix compose
// is loop-carried (horizon_selection.py:66-75); the stage blocks (:57-64) and the
// queries (:77-85) of different steps are independent.  So one workgroup takes one
// handed-over problem at a time, in beats of 64 steps:
//   wave 0: the stage blocks E_k, F_k, G_k of beat b, one step per lane;
//   wave 1: the compose chain of beat b - 1 (W_k and the prefix update), the same
//           values on every lane, W_k's LU slot column by column (spd_inverse_lanes);
//   wave 2: the queries of beat b - 2, one horizon per lane, then the argmin in
//           horizon order on lane 0.
// The blocks pass through two LDS rings of two beats.  Every value comes from the
// same small_math.hpp functions on the same inputs as in lft_small_kernel, so J, the
// status word and T* / J* are bitwise the one-lane kernel's (HOP_OPT_RERUN_LANE runs
// that instead; tests/test_gpu_small_rowgroup.py).  A workgroup with more than
// kSmallPipeMax hand-overs runs the one-lane body on all of them (64 lanes in
// parallel beat a sequence of pipelines there).
constexpr int kSmallPipeMax = 3;
// HOP_PIPE_SEQ_INV=1 (A/B): the chain's W_k by spd_inverse itself (no column-parallel LU)
#ifndef HOP_PIPE_SEQ_INV
#define HOP_PIPE_SEQ_INV 0
#endif
template <class T, int S, int MM>
struct PipeSmallGeo {
  static constexpr int NP = S * (S + 1) / 2, SS = S * S;
  static constexpr int STG = NP + SS + NP;  // E / Ebar, F / Fbar, G / Gbar of one step
  static constexpr int BS = 64;             // steps per beat (a wave's lanes)
  static constexpr int RING = 2 * BS * STG; // elements per ring (two beats)
  static constexpr int OFF_C = RING, OFF_J = 2 * RING;  // chain ring, the beat's J values
  static constexpr int BYTES = (2 * RING + BS) * (int)sizeof(T) + 16;  // + the status word
};

template <class T, int S>
__device__ __forceinline__ void put_step(T* o, const Sym<T, S>& e, const Gen<T, S>& f,
                                         const Sym<T, S>& g) {
  constexpr int NP = Sym<T, S>::NP;
#pragma unroll
  for (int i = 0; i < NP; ++i) o[i] = e.v[i];
#pragma unroll
  for (int i = 0; i < S; ++i)
#pragma unroll
    for (int j = 0; j < S; ++j) o[NP + i * S + j] = f.a[i][j];
#pragma unroll
  for (int i = 0; i < NP; ++i) o[NP + S * S + i] = g.v[i];
}
template <class T, int S>
__device__ __forceinline__ void get_step(const T* in, Sym<T, S>& e, Gen<T, S>& f, Sym<T, S>& g) {
  constexpr int NP = Sym<T, S>::NP;
#pragma unroll
  for (int i = 0; i < NP; ++i) e.v[i] = in[i];
#pragma unroll
  for (int i = 0; i < S; ++i)
#pragma unroll
    for (int j = 0; j < S; ++j) f.a[i][j] = in[NP + i * S + j];
#pragma unroll
  for (int i = 0; i < NP; ++i) g.v[i] = in[NP + S * S + i];
}

// spd_inverse (small_math.hpp: chol_inv's jitter ladder, then the LU slot) for the chain
// wave of the pipelined rerun, which calls it on all 64 lanes with the same input: the
// ladder runs as in spd_inverse on every lane, and the LU slot's five right-hand sides
// (the identity's columns) are solved side by side, lane c taking column c of the one
// factorisation (a column's operations do not depend on the others', so the values are
// lu_sym_solve_regs<T, S, S>'s bit for bit).  Running the ladder's attempts side by side
// as well (lane t at jitter t, the first that factors broadcast) was measured 27 %
// faster on the point-mass select but differs from the sequential ladder in the last
// bits of some steps (tools/dbg_handover.py), so it is not used.
template <class T, int S>
__device__ __forceinline__ T bcast_lane(T v, int src) {
  if constexpr (sizeof(T) == 8) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, src);
    const unsigned hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), src);
    return __builtin_bit_cast(T, ((unsigned long long)hi << 32) | lo);
  } else {
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(unsigned, v), src));
  }
}
template <class T, int S>
__device__ __forceinline__ void spd_inverse_lanes(Sym<T, S>& m, int max_tries, unsigned& st, int lane) {
  // the ladder as spd_inverse runs it (every lane the same attempts)
  const Sym<T, S> in = m;
  T eps = T(1e-9);
  bool ok = sweep_neg_inverse(m, eps);
  if (!ok && !all_finite(in)) {  // chol_inv's _assert_finite: no ladder
    st |= kStNonfinite;
#pragma unroll
    for (int k = 0; k < Sym<T, S>::NP; ++k) m.v[k] = T(__builtin_nan(""));
    return;
  }
  if (!ok) {
    st |= kStJitter;
    for (int tries = 1;; ++tries) {
      eps *= T(10);
      m = in;
      ok = sweep_neg_inverse(m, eps);
      if (ok) break;
      if (tries >= max_tries) {  // the LU slot: lane c solves the identity's column c
        st |= kStLu;
        const int col = lane < S ? lane : S - 1;
        T x[S][1];
#pragma unroll
        for (int i = 0; i < S; ++i) x[i][0] = i == col ? T(1) : T(0);
        const bool okl =
            lu_sym_solve_regs<T, S, 1>([&](int i, int j) { return in.at(i, j); }, eps, x);
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
          for (int j = i; j < S; ++j)
            m.at(i, j) = okl ? -bcast_lane<T, S>(x[i][0], j) : T(__builtin_nan(""));
        break;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < Sym<T, S>::NP; ++k) m.v[k] = -m.v[k];
}

template <class T, int S, int MM>
__device__ __forceinline__ void pipe_small_problem(const LftArgs<T>& a, long long p, int w, int lane,
                                                   T* ring, unsigned* st_all) {
  using PG = PipeSmallGeo<T, S, MM>;
  constexpr int SS = S * S, BS = PG::BS, STG = PG::STG;
  const int N = a.n, mt = a.max_tries;
  const long long pstrM = (long long)a.nalloc * SS, pstrB = (long long)a.nalloc * S * MM;
  if (threadIdx.x == 0) *st_all = 0u;
  __syncthreads();
  unsigned st = 0;
  T rinv[MM][MM];
  if (w == 0) {  // R^-1 as the one-lane kernel forms it (its status bits included)
    const T* Rp = a.R + p * a.r_bstride;
    Gen<T, MM> r;
#pragma unroll
    for (int i = 0; i < MM; ++i)
#pragma unroll
      for (int j = 0; j < MM; ++j) r.a[i][j] = Rp[i * MM + j];
    Sym<T, MM> rs;
    sym_of(rs, r);
    if (!a.r_is_inv) spd_inverse(rs, mt, st);
#pragma unroll
    for (int i = 0; i < MM; ++i)
#pragma unroll
      for (int j = 0; j < MM; ++j) rinv[i][j] = a.r_is_inv ? r.a[i][j] : rs.at(i, j);
  }
  T z[S];
  if (w == 2) {
#pragma unroll
    for (int i = 0; i < S; ++i) z[i] = a.z0[p * a.z_bstride + i];
  }
  State<T, S, MM> ch;  // wave 1, lane 0: the prefix
  ch.st = 0;
  State<T, S, MM> am;  // wave 2, lane 0: the argmin (take)
  am.st = 0;
  am.best = T(0);
  am.tbest = 0;
  T* jb = ring + PG::OFF_J;
  const int nb = (N + BS - 1) / BS;
#pragma unroll 1
  for (int beat = 0; beat < nb + 2; ++beat) {
    if (w == 0) {
      const int k = beat * BS + lane;
      if (beat < nb && k < N) {
        Gen<T, S> Q, A;
        T Bk[S][MM];
        const T* q = a.Q + p * pstrM + (long long)k * SS;
        const T* ap = a.A + p * pstrM + (long long)k * SS;
        const T* bp = a.B + p * pstrB + (long long)k * S * MM;
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
          for (int j = 0; j < S; ++j) {
            Q.a[i][j] = q[i * S + j];
            A.a[i][j] = ap[i * S + j];
          }
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
          for (int j = 0; j < MM; ++j) Bk[i][j] = bp[i * MM + j];
        Sym<T, S> E, G;
        Gen<T, S> F;
        stage_blocks<T, S, MM>(Q, A, Bk, rinv, mt, st, E, F, G);
        put_step<T, S>(ring + ((beat & 1) * BS + lane) * STG, E, F, G);
      }
    } else if (w == 1) {
      const int b1 = beat - 1;
      if (b1 >= 0 && b1 < nb) {  // every lane carries the same prefix
#pragma unroll 1
        for (int j = 0; j < BS; ++j) {
          const int k = b1 * BS + j;
          if (k >= N) break;
          Sym<T, S> E, G;
          Gen<T, S> F;
          get_step<T, S>(ring + ((b1 & 1) * BS + j) * STG, E, F, G);
#if HOP_PIPE_SEQ_INV
          compose_step<T, S, MM>(ch, k, E, F, G, mt);
#else
          compose_step<T, S, MM>(ch, k, E, F, G, mt, [&](Sym<T, S>& x, int t, unsigned& s_) {
            spd_inverse_lanes<T, S>(x, t, s_, lane);
          });
#endif
          if (lane == 0)
            put_step<T, S>(ring + PG::OFF_C + ((b1 & 1) * BS + j) * STG, ch.Eb, ch.Fb, ch.Gb);
        }
      }
    } else if (w == 2) {
      const int b2 = beat - 2;
      if (b2 >= 0) {  // (b2 < nb: the loop ends at nb + 2)
        const int k = b2 * BS + lane;
        if (k < N) {
          State<T, S, MM> s;
          s.st = 0;
          get_step<T, S>(ring + PG::OFF_C + ((b2 & 1) * BS + lane) * STG, s.Eb, s.Fb, s.Gb);
          Gen<T, S> QT;
          const T* qt = a.QT + p * pstrM + (long long)k * SS;
#pragma unroll
          for (int i = 0; i < S; ++i)
#pragma unroll
            for (int j = 0; j < S; ++j) QT.a[i][j] = qt[i * S + j];
          const T jk = query<T, S, MM>(s, QT, z, mt);
          st |= s.st;
          a.J[p * N + k] = jk;
          jb[lane] = jk;
        }
        wave_sync();
        if (lane == 0) {
#pragma unroll 1
          for (int j = 0; j < BS; ++j) {
            const int kk = b2 * BS + j;
            if (kk >= N) break;
            take(am, kk + 1, jb[j], a.t_min, a.t_max);
          }
        }
      }
    }
    __syncthreads();
  }
  if (w == 1 && lane == 0) st |= ch.st;
  if (w == 2 && lane == 0) st |= am.st;
  if (st != 0u) atomicOr(st_all, st);
  __syncthreads();
  if (w == 2 && lane == 0) {
    a.status[p] = (int)*st_all;
    if (a.t_max > 0 && a.t_star != nullptr) {
      a.t_star[p] = am.tbest;
      a.j_star[p] = am.best;
    }
  }
  __syncthreads();  // the next problem reuses the rings and the status word
}

// The rerun launch after the conditioned small-s kernels (kCondRerun): the
// workgroup's hand-overs (status 16) by the pipeline when there are at most
// kSmallPipeMax of them, else by the one-lane body
template <class T, int S, int MM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1))) void lft_small_rerun_kernel(LftArgs<T> a) {
  using G = Geo<T, S, MM>;
  using PG = PipeSmallGeo<T, S, MM>;
  static_assert(G::WPB >= 3, "the pipeline needs three waves per workgroup");
  static_assert(PG::BYTES <= G::WAVE_BYTES * G::WPB, "the rings must fit the LFT kernel's LDS");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  if (!(a.cond & kCondRerun)) {  // HOP_OPT_REFERENCE_ASSOC: every problem, one per lane
    lft_small_body<T, S, MM, false, 64, 0, 1>(a);
    return;
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long prob = (long long)blockIdx.x * G::PPB + w * 64 + lane;
  const bool need = prob < a.batch && (a.status[prob] & 16);
  unsigned long long* masks = reinterpret_cast<unsigned long long*>(smem_raw);
  const unsigned long long bal = __ballot(need);
  if (lane == 0) masks[w] = bal;
  __syncthreads();
  unsigned long long mk[G::WPB];
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < G::WPB; ++i) {
    mk[i] = masks[i];
    cnt += __popcll(mk[i]);
  }
  if (cnt == 0) return;  // workgroup-uniform
  // the masks live where the rings and the body's LDS-DMA images go: every wave has
  // read them before either branch writes there (cnt is workgroup-uniform)
  __syncthreads();
  if (cnt > kSmallPipeMax) {
    lft_small_body<T, S, MM, false, 64, 0, 1>(a);
    return;
  }
  T* ring = reinterpret_cast<T*>(smem_raw);
  unsigned* st_all = reinterpret_cast<unsigned*>(smem_raw + (2 * PG::RING + PG::BS) * sizeof(T));
#pragma unroll 1
  for (int i = 0; i < G::WPB; ++i) {
    unsigned long long m = mk[i];
#pragma unroll 1
    while (m != 0ull) {
      const int l = __ffsll((long long)m) - 1;
      m &= m - 1ull;
      pipe_small_problem<T, S, MM>(a, (long long)blockIdx.x * G::PPB + i * 64 + l, w, lane, ring,
                                   st_all);
    }
  }
}


// ---------------------------------------------------------------------------
// Trajectory form (augmented.py:10-87 inside the sweep): the wave streams the
// raw A_k, B_k, x_{k+1}, a_k, u_k (chunk-major, as above) and every lane builds
// its augmented blocks in registers.  Only e_{k+1} is new each step: Q e_k and
// e_k^T Q e_k are carried from the previous step.
// LY 0: batch-major raw arrays (chunk-major pieces: piece r = the r-th 16-B chunk of
// every lane's block); LY 2: the tile64 layout [B/64][n_alloc (+1 for X)][elems][64]
// (include/hop.h), whose step block of the wave's 64 problems is one contiguous span
// (pieces = its consecutive KiB; the same piece counts, since a piece holds 64 x 16 B
// either way).  LAST_*: lanes of a section's last, partial tile64 piece.
template <class T, int S, int MM>
struct GeoT {
  static constexpr int NN = S - 1, TS = (int)sizeof(T);
  static constexpr int CA = (NN * NN * TS + 15) / 16, CB = (NN * MM * TS + 15) / 16;
  static constexpr int CX = (NN * TS + 15) / 16, CU = (MM * TS + 15) / 16;
  static constexpr int P_A = 0, P_B = CA, P_X = CA + CB, P_V = P_X + CX, P_U = P_V + CX;
  static constexpr int PIECES = P_U + CU;
  static constexpr int WAVE_BYTES = PIECES * 1024;
  static constexpr int WPB = 4, TPB = 256, PPB = 256;
  static constexpr int LAST_A = (64 * NN * NN * TS - (CA - 1) * 1024) / 16;
  static constexpr int LAST_B = (64 * NN * MM * TS - (CB - 1) * 1024) / 16;
  static constexpr int LAST_X = (64 * NN * TS - (CX - 1) * 1024) / 16;
  static constexpr int LAST_U = (64 * MM * TS - (CU - 1) * 1024) / 16;
};

template <class T, int S, int MM, bool COND = false, int LY = 0>
__global__ __launch_bounds__(256, 1) void lft_small_traj_kernel(LftArgs<T> a) {
  static_assert(LY == 0 || LY == 2, "batch-major or tile64 raw arrays");
  using G = GeoT<T, S, MM>;
  constexpr int NN = G::NN, TS = G::TS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned char* wimg = smem_raw + w * G::WAVE_BYTES;
  const unsigned wlds = (unsigned)(uintptr_t)wimg;
  const long long wave_prob0 = (long long)blockIdx.x * G::TPB + w * 64;
  const long long prob = wave_prob0 + lane;
  bool valid = prob < a.batch;
  const long long pb = valid ? prob : a.batch - 1;
  if (wave_prob0 >= a.batch) return;  // wave-uniform; no workgroup barrier in this kernel
  const long long pb0 = wave_prob0;
  if (!COND && (a.cond & kCondRerun)) {  // rerun launch (see lft_small_kernel)
    const bool need = valid && (a.status[prob] & 16);
    if (!__any(need)) return;
    valid = need;
  }
  const int N = a.n, mt = a.max_tries, NA = a.nalloc;
  const TrajArgs<T>& t = a.tr;
  const long long pA = (long long)NA * NN * NN * TS, pB = (long long)NA * NN * MM * TS;
  const long long pX = (long long)(NA + 1) * NN * TS, pV = (long long)NA * NN * TS;
  const long long pU = (long long)NA * MM * TS;
  auto mk = [&](const T* base, long long pstr) {  // exact bounds (per-dword range check)
    // tile64: the wave's tile is allocated whole (padding slots included)
    const long long left = (LY == 2 ? 64 : a.batch - pb0) * pstr;
    const unsigned nrec = left > 0xFFFFFFF0ll ? 0xFFFFFFF0u : (unsigned)left;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(base) + pb0 * (pstr / TS), (short)0,
                                             (int)nrec, 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t rA = mk(t.A, pA), rB = mk(t.Bm, pB), rX = mk(t.X, pX),
                               rV = mk(t.ares, pV), rU = mk(t.U, pU);
  // lane source offsets: LY 0 the lane's own problem (+ 16 r per chunk), LY 2 the
  // lane's 16 B of the step's contiguous tile span (+ 1024 r per piece)
  const unsigned lo = 16u * lane;
  const unsigned vA = LY == 2 ? lo : (unsigned)((pb - pb0) * pA),
                 vB = LY == 2 ? lo : (unsigned)((pb - pb0) * pB),
                 vX = LY == 2 ? lo : (unsigned)((pb - pb0) * pX),
                 vV = LY == 2 ? lo : (unsigned)((pb - pb0) * pV),
                 vU = LY == 2 ? lo : (unsigned)((pb - pb0) * pU);
  constexpr unsigned RS = LY == 2 ? 1024u : 16u;  // source stride between pieces
  constexpr unsigned KS = LY == 2 ? 64u : 1u;     // step stride factor (64 problems)
  auto dma_step = [&](int k) {  // A_k, B_k, x_{k+1}, a_k, u_k
    const unsigned sA = (unsigned)(k * NN * NN * TS) * KS, sB = (unsigned)(k * NN * MM * TS) * KS,
                   sX = (unsigned)((k + 1) * NN * TS) * KS, sV = (unsigned)(k * NN * TS) * KS,
                   sU = (unsigned)(k * MM * TS) * KS;
    // tile64: a section's last piece is partial; its lanes past the data would write
    // the next step's elements into the following image, so they issue nothing; the
    // full pieces go four to an M0 (dma_block64v)
    if constexpr (LY == 2) {
      dma_block64v<G::CA, G::LAST_A>(vA, rA, wlds + G::P_A * 1024u, sA, lane);
      dma_block64v<G::CB, G::LAST_B>(vB, rB, wlds + G::P_B * 1024u, sB, lane);
      dma_block64v<G::CX, G::LAST_X>(vX, rX, wlds + G::P_X * 1024u, sX, lane);
      dma_block64v<G::CX, G::LAST_X>(vV, rV, wlds + G::P_V * 1024u, sV, lane);
      dma_block64v<G::CU, G::LAST_U>(vU, rU, wlds + G::P_U * 1024u, sU, lane);
      return;
    }
#pragma unroll
    for (int r = 0; r < G::CA; ++r)
      if (LY != 2 || r + 1 < G::CA || lane < G::LAST_A)
        dma16(vA + RS * r, rA, wlds + (G::P_A + r) * 1024, sA);
#pragma unroll
    for (int r = 0; r < G::CB; ++r)
      if (LY != 2 || r + 1 < G::CB || lane < G::LAST_B)
        dma16(vB + RS * r, rB, wlds + (G::P_B + r) * 1024, sB);
#pragma unroll
    for (int r = 0; r < G::CX; ++r)
      if (LY != 2 || r + 1 < G::CX || lane < G::LAST_X)
        dma16(vX + RS * r, rX, wlds + (G::P_X + r) * 1024, sX);
#pragma unroll
    for (int r = 0; r < G::CX; ++r)
      if (LY != 2 || r + 1 < G::CX || lane < G::LAST_X)
        dma16(vV + RS * r, rV, wlds + (G::P_V + r) * 1024, sV);
#pragma unroll
    for (int r = 0; r < G::CU; ++r)
      if (LY != 2 || r + 1 < G::CU || lane < G::LAST_U)
        dma16(vU + RS * r, rU, wlds + (G::P_U + r) * 1024, sU);
  };
  auto vm_wait = []() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };

  // per-lane constants: raw Q (for Q e), _sym(Q) + q_reg I, P, xg, u_ref, 2w
  T Qr[NN][NN], Qt[NN][NN], Pm[NN][NN], xg[NN], ur[MM];
  {
    const T* Qg = t.Q + pb * t.q_bs;
    const T* Pg = t.P + pb * t.p_bs;
#pragma unroll
    for (int i = 0; i < NN; ++i)
#pragma unroll
      for (int j = 0; j < NN; ++j) {
        Qr[i][j] = Qg[i * NN + j];
        Pm[i][j] = Pg[i * NN + j];
      }
#pragma unroll
    for (int i = 0; i < NN; ++i)
#pragma unroll
      for (int j = 0; j < NN; ++j)
        Qt[i][j] = T(0.5) * (Qr[i][j] + Qr[j][i]) + (i == j ? t.q_reg : T(0));
#pragma unroll
    for (int i = 0; i < NN; ++i) xg[i] = t.xg[pb * t.xg_bs + i];
#pragma unroll
    for (int q = 0; q < MM; ++q) ur[q] = t.u_ref[pb * t.ur_bs + q];
  }
  const T w2 = T(2) * t.w[pb * t.w_bs], rho = t.rho_reg;
  auto err = [&](const T (&x)[NN], T (&e)[NN]) {  // wrap_error(x - xg) (utils.py:131-137)
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      const T d = x[i] - xg[i];
      e[i] = ((t.wrap_mask >> i) & 1u) ? wrap_angle(d) : d;
    }
  };
  auto quad_of = [&](const T (&M)[NN][NN], const T (&e)[NN], T (&me)[NN]) {  // M e, e^T M e
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      T v = T(0);
#pragma unroll
      for (int j = 0; j < NN; ++j) v += M[i][j] * e[j];
      me[i] = v;
    }
    T s2 = T(0);
#pragma unroll
    for (int j = 0; j < NN; ++j) s2 += e[j] * me[j];
    return s2;
  };
  T qe[NN], eqe;  // Q e_k, e_k^T Q e_k
  {
    T x0[NN], e0[NN];
    // x_0: batch-major row 0 of the problem, or tile64 element i of step 0 of its tile
    const T* Xg = LY == 2 ? t.X + (pb >> 6) * (long long)(NA + 1) * NN * 64 + (pb & 63)
                          : t.X + pb * (long long)(NA + 1) * NN;
#pragma unroll
    for (int i = 0; i < NN; ++i) x0[i] = Xg[LY == 2 ? 64 * i : i];
    err(x0, e0);
    eqe = quad_of(Qr, e0, qe);
  }
  T z[S];
#pragma unroll
  for (int i = 0; i < S; ++i) z[i] = i == NN ? T(1) : T(0);  // z0 = e_s (augmented.py:57)
  State<T, S, MM> ps;
  ps.st = 0;
  ps.best = T(0);
  ps.tbest = 0;
  CondState<T, S, MM> cs;
  if constexpr (COND) {
    cond_init(cs, z);
    cs.bad = (a.cond & kCondFlagAll) != 0;
    cs.kf1 = cs.bad ? 1 : 0;
  }
  T rinv[MM][MM];  // R_inv_cached
  {
    const T* Rp = a.R + pb * a.r_bstride;
#pragma unroll
    for (int i = 0; i < MM; ++i)
#pragma unroll
      for (int j = 0; j < MM; ++j) rinv[i][j] = Rp[i * MM + j];
  }
  if (N > 0) dma_step(0);
  constexpr int JR = 8;  // J ring, as lft_small_kernel
  T jring[JR];
#pragma unroll
  for (int i = 0; i < JR; ++i) jring[i] = T(0);
  auto flush = [&](int k0, int cnt) {
    if (valid) {
#pragma unroll
      for (int i = 0; i < JR; ++i)
        if (i >= JR - cnt) a.J[prob * N + k0 + i - (JR - cnt)] = jring[i];
    }
  };
#pragma unroll 1
  for (int k = 0; k < N; ++k) {
    vm_wait();
    wave_sync();
    if (k >= JR && k % JR == 0) flush(k - JR, JR);
    T Ar[NN][NN], Br[NN][MM], x1[1][NN], av[1][NN], uu[1][MM];
    read_block<T, NN, NN, G::P_A, 1024, LY>(wimg, lane, Ar);
    read_block<T, NN, MM, G::P_B, 1024, LY>(wimg, lane, Br);
    read_block<T, 1, NN, G::P_X, 1024, LY>(wimg, lane, x1);
    read_block<T, 1, NN, G::P_V, 1024, LY>(wimg, lane, av);
    read_block<T, 1, MM, G::P_U, 1024, LY>(wimg, lane, uu);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (k + 1 < N) dma_step(k + 1);
    // augmented blocks of step k (augmented.py:31-56, 77-86; the final _sym is exact)
    Gen<T, S> Qk, Ak, QTk;
    T Bk[S][MM];
    T e1[NN], pe[NN], qe1[NN];
    err(x1[0], e1);
    const T epe = quad_of(Pm, e1, pe);
    const T eqe1 = quad_of(Qr, e1, qe1);
    T du[MM];
#pragma unroll
    for (int q = 0; q < MM; ++q) du[q] = uu[0][q] - ur[q];
#pragma unroll
    for (int i = 0; i < NN; ++i) {
#pragma unroll
      for (int j = 0; j < NN; ++j) {
        Qk.a[i][j] = Qt[i][j];
        QTk.a[i][j] = Pm[i][j];
        Ak.a[i][j] = Ar[i][j];
      }
      Qk.a[i][NN] = Qk.a[NN][i] = qe[i];
      QTk.a[i][NN] = QTk.a[NN][i] = pe[i];
      T bd = T(0);
#pragma unroll
      for (int q = 0; q < MM; ++q) {
        bd += Br[i][q] * du[q];
        Bk[i][q] = Br[i][q];
      }
      Ak.a[i][NN] = av[0][i] - bd;
      Ak.a[NN][i] = T(0);
    }
    Qk.a[NN][NN] = (eqe + w2) + rho;
    QTk.a[NN][NN] = epe + rho;
    Ak.a[NN][NN] = T(1);
#pragma unroll
    for (int q = 0; q < MM; ++q) Bk[NN][q] = T(0);
    T jk;
    if constexpr (COND) {
      Sym<T, S> E;
      sym_of(E, Qk);
      cs.bad = cs.bad || !spd_inverse_once(E);
      cond_step<T, S, MM>(cs, E, Ak, Bk, rinv);
      jk = cond_query<T, S, MM>(cs, QTk);
    } else {
      stage_compose<T, S, MM>(ps, k, Qk, Ak, Bk, rinv, mt);
      jk = query<T, S, MM>(ps, QTk, z, mt);
    }
#pragma unroll
    for (int i = 0; i + 1 < JR; ++i) jring[i] = jring[i + 1];
    jring[JR - 1] = jk;
    if constexpr (COND) {
      take(cs, k + 1, jk, a.t_min, a.t_max);
      cond_mark(cs, k);
    } else {
      take(ps, k + 1, jk, a.t_min, a.t_max);
    }
#pragma unroll
    for (int i = 0; i < NN; ++i) qe[i] = qe1[i];
    eqe = eqe1;
  }
  vm_wait();
  if (N > 0) {
    const int tail = N % JR == 0 ? JR : N % JR;
    flush(N - tail, tail);
  }
  if (valid) {
    if constexpr (COND) {
      a.status[prob] = cond_status_word(cs);
      if (a.t_max > 0 && a.t_star != nullptr) {
        a.t_star[prob] = cs.tbest;
        a.j_star[prob] = cs.best;
      }
    } else {
      a.status[prob] = (int)ps.st;
      if (a.t_max > 0 && a.t_star != nullptr) {
        a.t_star[prob] = ps.tbest;
        a.j_star[prob] = ps.best;
      }
    }
  }
}

// launch shape of a geometry: dynamic LDS per block, problems and threads per block
struct LaunchGeo {
  int bytes, ppb, tpb;
};
template <class G>
constexpr LaunchGeo geo_of() {
  return {G::WAVE_BYTES * G::WPB, G::PPB, G::TPB};
}

// the rerun launch's kernel for batch-major blocks: the pipelined rerun for fp64
// (HOP_OPT_RERUN_LANE: the one-lane LFT kernel, its comparator), the one-lane LFT
// kernel for fp32 (whose conditioned association runs on the lane kernel too)
template <class T, int S, int MM>
auto rerun_kernel() {
  if constexpr (sizeof(T) == 8) {
    if (!opt(HOP_OPT_RERUN_LANE)) return &lft_small_rerun_kernel<T, S, MM>;
  }
  return &lft_small_kernel<T, S, MM, false, 64, 0, 1>;
}

}  // namespace small

// small-s path: returns hipErrorNotSupported when the shape has no instantiation
template <class T>
hipError_t dispatch_lft_small(const LftArgs<T>& a, hipStream_t stream) {
  if (a.dbg_efg || a.dbg_pre || a.r_kstride != 0) return hipErrorNotSupported;
  if (a.traj && (a.tr.n != a.s - 1 || a.tr.m != a.m || !a.r_is_inv)) return hipErrorNotSupported;
  // Batch-major blocks stream as problem-major pieces (LY 1); tile64 blocks (LY 2)
  // as contiguous 1-KiB pieces.  The batch-major stream is the bound at config 3:
  // its DMA alone takes 1.54 ms, the tile64 one 0.80 ms (tools/exp_tiled.py).
  // Every small-s shape, both layouts and both dtypes: the conditioned association
  // (half the FLOPs; at config 3 its stream, not its arithmetic, is the bound:
  // 0.83 ms against 0.91 for the LFT and 0.81 for the stream alone), then the LFT
  // kernel in rerun mode for the problems it handed over (chol_inv ladders, status
  // bits: the reference's semantics).  On real s = 5 linearisations at rho_reg =
  // 1e-12 the conditioned form holds the 50-digit reference curve where the fp64
  // reference association is 1e-2 .. 1 off, so augmented blocks and
  // the trajectory form run the same arithmetic.  HOP_OPT_REFERENCE_ASSOC: the LFT
  // kernel alone (the reference association; comparator for the tests and tools).
  // Developer builds: variant 62 the COND kernel alone (A/B), 79 the trajectory form's
  // LFT association alone, and the layout / occupancy experiments (72-78).
  // The conditioned step's loop-carried chain is no shorter than the LFT's
  using small::LaunchGeo;
  auto launch = [&](auto kern, LaunchGeo g, const LftArgs<T>& args) {
    const long long blocks = (a.batch + g.ppb - 1) / g.ppb;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3((unsigned)g.tpb), (size_t)g.bytes, stream,
                       args);
    return hipGetLastError();
  };
  auto go1 = [&](auto kl, LaunchGeo g) { return launch(kl, g, a); };
  const int variant = kDevBuild ? g_opt_variant : 0;
  const bool ref = opt(HOP_OPT_REFERENCE_ASSOC);
  const bool ref_traj = ref || variant == 79;  // 79: the trajectory form's LFT association
  const bool exp78 = ref && variant == 78;     // 78: a tile64 layout experiment (LFT kernel)
  // the launch pair (kCondPolicyPlain, hop_kernels.hpp).  lft_only: the LFT kernel
  // alone with the caller's word, which is also how the hand-overs of lft_sweep_v2.hip's
  // small-s row-group kernel arrive (kCondRerunOnly: this dispatcher's rerun launch alone)
  auto gopair = [&](auto kc, auto kl, LaunchGeo g, bool lft_only) {
    if (lft_only || (a.cond & kCondRerunOnly)) return go1(kl, g);
    CondPolicy p = kCondPolicyPlain;
    p.rerun = variant != 62;
    return launch_cond_pair(
        a, p, [&](const LftArgs<T>& c) { return launch(kc, g, c); },
        [&](const LftArgs<T>& r) { return launch(kl, g, r); });
  };
#define HOP_SMALL_TRAJ(S_, M_)                                                            \
  if (a.traj && a.s == S_ && a.m == M_)                                                   \
    return a.tile64 ? gopair(small::lft_small_traj_kernel<T, S_, M_, true, 2>,            \
                             small::lft_small_traj_kernel<T, S_, M_, false, 2>,           \
                             small::geo_of<small::GeoT<T, S_, M_>>(), ref_traj)           \
                    : gopair(small::lft_small_traj_kernel<T, S_, M_, true, 0>,            \
                             small::lft_small_traj_kernel<T, S_, M_, false, 0>,           \
                             small::geo_of<small::GeoT<T, S_, M_>>(), ref_traj);
#ifdef HOP_DEV
  // variant 78 (tile64, reference association), 74-77 (batch-major): layout experiments
  // of the LFT kernel; 72: 32 problems per wave (two waves per SIMD), A/B against 64;
  // 73: the conditioned association at 32 problems per wave + the rerun launch
#define HOP_SMALL_DEV(S_, M_)                                                             \
  if (a.tile64) /* only exp78 comes here with tile64 blocks */                            \
    return go1(small::lft_small_kernel<T, S_, M_, false, 64, 1, 2>,                       \
               small::geo_of<small::Geo<T, S_, M_>>());                                   \
  if (variant == 72)                                                                      \
    return go1(small::lft_small_kernel<T, S_, M_, false, 32>,                             \
               small::geo_of<small::Geo<T, S_, M_, 32>>());                               \
  if (variant == 74 || variant == 75)                                                     \
    return go1(variant == 74 ? small::lft_small_kernel<T, S_, M_, false, 64, 1>           \
                             : small::lft_small_kernel<T, S_, M_, false, 64, 2>,          \
               small::geo_of<small::Geo<T, S_, M_>>());                                   \
  if (variant == 76)                                                                      \
    return go1(small::lft_small_kernel<T, S_, M_, false, 64, 0, 0>,                       \
               small::geo_of<small::Geo<T, S_, M_>>());                                   \
  if (variant == 77)                                                                      \
    return go1(small::lft_small_kernel<T, S_, M_, false, 64, 1, 1>,                       \
               small::geo_of<small::Geo<T, S_, M_>>());                                   \
  if (variant == 73)                                                                      \
    return gopair(small::lft_small_kernel<T, S_, M_, true, 32>,                           \
                  small::lft_small_kernel<T, S_, M_, false, 32>,                          \
                  small::geo_of<small::Geo<T, S_, M_, 32>>(), ref);
#else
#define HOP_SMALL_DEV(S_, M_)
#endif
#define HOP_SMALL(S_, M_)                                                                 \
  HOP_SMALL_TRAJ(S_, M_)                                                                  \
  if (a.s == S_ && a.m == M_) {                                                           \
    if (a.tile64 && !exp78)                                                               \
      return gopair(small::lft_small_kernel<T, S_, M_, true, 64, 0, 2>,                   \
                    small::lft_small_kernel<T, S_, M_, false, 64, 0, 2>,                  \
                    small::geo_of<small::Geo<T, S_, M_>>(), ref);                         \
    HOP_SMALL_DEV(S_, M_)                                                                 \
    return gopair(small::lft_small_kernel<T, S_, M_, true, 64, 0, 1>,                     \
                  small::rerun_kernel<T, S_, M_>(),                                       \
                  small::geo_of<small::Geo<T, S_, M_>>(), ref);                           \
  }
  HOP_SMALL(2, 1) HOP_SMALL(3, 1) HOP_SMALL(4, 1) HOP_SMALL(4, 2) HOP_SMALL(5, 1)
  HOP_SMALL(5, 2)  // fp32 s = 6 spills: generic kernel
#undef HOP_SMALL
#undef HOP_SMALL_DEV
#undef HOP_SMALL_TRAJ
  return hipErrorNotSupported;
}

template hipError_t dispatch_lft_small<float>(const LftArgs<float>&, hipStream_t);
template hipError_t dispatch_lft_small<double>(const LftArgs<double>&, hipStream_t);

}  // namespace hop
