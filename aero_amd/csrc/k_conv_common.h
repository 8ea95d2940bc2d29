// k_conv_common.h -- launch parameters and LDS tile addressing shared by the convolution kernels (k_conv.h, k_conv_ring.h)
#pragma once
#include "aero_common.h"

struct AeroConvK {
    aero_conv_desc d;
    int Cp, cpt, Ktot, Mpad, nmt, ntt, vec_in, vec4, vec_out, staged, glds;
    int nT, f_lo, f_step, t_lo, t_step;      // regular tap grid: df = f_lo + (j / nT) * f_step, dt = t_lo + (j % nT) * t_step
    int tsplit;                              // >= 1: groups the time taps are split into (aero_conv_desc.tap_split)
};

// Host side of one aero_conv_fwd (k_conv.h; the ring tile's share in k_conv_ring.h): aero_conv_plan routes the descriptor to a kernel family and
// instantiation and fills the AeroConvK fields that kernel reads, aero_conv_issue launches what the plan says, aero_conv_plan_name prints it
enum AeroConvFamily { AERO_CONV_TINY, AERO_CONV_CARRY, AERO_CONV_STREAM, AERO_CONV_SKINNY, AERO_CONV_RING, AERO_CONV_GLDS8, AERO_CONV_GLDS, AERO_CONV_GENERIC };
struct AeroConvPlan {
    AeroConvFamily family;
    int t[4];                                // template integers: carry {NCH}, skinny {VW}, ring {WM, WN, NRB, NT}, glds8 {MF}, glds {MF, WM, KC}, generic {MF, WM}
    bool stats;                              // glds8 / glds / generic: the STATS instantiation
    unsigned grid, block;
    size_t lds;                              // dynamic LDS bytes
    int QC;                                  // carry: source rows per chunk of a wave
    void tile(AeroConvFamily f, int a = 0, int b = 0, int c = 0, int e = 0) { family = f; t[0] = a; t[1] = b; t[2] = c; t[3] = e; }
    bool is(int a, int b = 0, int c = 0, int e = 0) const { return t[0] == a && t[1] == b && t[2] == c && t[3] == e; }
};

static inline int aero_env_on(const char* e) { return (e && e[0] == '0') ? 0 : 1; }     // environment switches: on unless the value starts with '0'
static inline int aero_env_int(const char* e, int dflt) { return e ? atoi(e) : dflt; }  // ... and integers with a default

// LDS image of a [rows][KC] fp16 operand tile: 16-byte slot `slot` of row `row`, XOR-swizzled so that the ds_read_b128
// fragment reads of both MFMA shapes (16x16x32: lane -> row l&15, slot l>>4; 32x32x16: row l&31, slot 2*ks + (l>>5)) are
// bank-conflict free.  The direct global->LDS copies write lane-linear, so the permutation goes on the SOURCE address.
template <int KC>
static __device__ __forceinline__ int aero_tile_off_kc(int row, int slot) {
    if (KC == 32) return row * 32 + ((slot ^ ((0 - (row >> 2)) & 3)) << 3);
    return row * 64 + ((slot ^ ((row >> 1) & 7)) << 3);
}
template <int KC>
static __device__ __forceinline__ int aero_tile_swz(int row) {
    return KC == 32 ? ((0 - (row >> 2)) & 3) : ((row >> 1) & 7);
}

