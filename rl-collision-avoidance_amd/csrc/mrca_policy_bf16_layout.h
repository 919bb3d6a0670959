// mrca_policy_bf16_layout.h -- LDS image and operand address formulas of the bf16 front end (csrc/mrca_policy_bf16.hip,
// namespace mrca_pbf16).  Plain integer functions, shared by the gfx950 kernel and by the CPU test
// (tests/test_policy_bf16_layout.py compiles a shim around this header and re-enacts one wave's data movement with it).
//
// One wave owns one (robot, tower) at a time.  Its image is ONE region of kWaveBytes, used three ways in turn:
//   H[kHRows][32] bf16   relu(conv1) position-major: H[p + 1][c] = h1[c][p] (p < 255), H[0] = H[256] = 0 (conv2's paddings).
//                        Rows of 64 B: the 8 channels a lane needs of one position are one 16-byte read.
//   X[kXRows][4] bf16    the scan position-major, at byte kXOff INSIDE H: X[i + 1][ci] = x[ci][i], X[0] = x[.][-1] = 0,
//                        channel 3 = 0.  conv1's tile T reads X rows [64 T, 64 T + 66] and writes H rows [32 T + 1, 32 T + 32];
//                        kXOff puts every X row a later tile reads above every H row an earlier tile wrote
//                        (x_alias_ok below), so the scan needs no space of its own.
//   O[32][kOPitch] bf16  feat of the finished (robot, tower), channel-major, at byte kOOff inside H (written once conv2 has
//                        read all of H): the accumulators (channel on the lane) go in as 8-byte rows of 4 positions, 16-byte
//                        rows of 8 positions come out and go to HBM as they are.  Below X and above H[0].
// Before the first robot the same region holds the tower's fp32 weights for one pass (W2L / W1L, padded odd pitches).
//
// MFMA mapping (v_mfma_f32_32x32x16_bf16; lane l, r = l & 31, hl = l >> 5; A[r][8 hl + j], B[8 hl + j][r], j < 8):
//   conv1  C[32 ch][32 pos] = W1 x X1, two MFMAs per tile of 32 positions (8 tiles, position 255 computed and dropped):
//          mf 0: k = 8 hl + j <-> tap 2 hl + (j >> 2), ci = j & 3        B = 16 bytes at X row 2p + 2 hl
//          mf 1: k = j (hl = 0, j < 4) <-> tap 4, ci = j; else zero      B =  8 bytes at X row 2p + 4
//          (ci = 3 is X's zero channel and a zero weight).  C: lane = position, registers = channels rowmap(r, hl).
//   conv2  C[32 pos][32 ch] = X2^T x W2^T, 6 k-steps per tile of 32 positions (4 tiles):
//          step s: k = 8 hl + j <-> tap s >> 1, ci = 16 (s & 1) + 8 hl + j      A = 16 bytes at H row 2l + tap
//          C: lane = channel, registers = positions rowmap(r, hl) of the tile -- four runs of 4 positions.
#pragma once

#if defined(__HIPCC__)
#define MRCA_PB_HD __host__ __device__ constexpr
#else
#define MRCA_PB_HD constexpr
#endif

namespace mrca_pbf16 {

constexpr int kBeams = 512, kFrames = 3, kCh = 32;
constexpr int kL1 = 255, kL2 = 128;

constexpr int kHRowBytes = 64;                     // 32 channels x 2 B
constexpr int kHRows = 257;                        // h1[.][-1], h1[.][0..254], h1[.][255]
constexpr int kWaveBytes = kHRows * kHRowBytes;    // 16 448 B: 9 waves per CU by LDS
constexpr int kXRowBytes = 8;                      // 3 channels + a zero, 2 B each
constexpr int kXRows = 515;                        // rows 0..514 (tile 7's dropped position 255 reads row 514)
constexpr int kXOff = 10816;
constexpr int kOPitch = 136;                       // bf16 per O row: 128 + 8 (16-byte aligned rows)
constexpr int kOOff = 64;
constexpr int kW2LPitch = 97, kW1LPitch = 17;      // fp32 weight staging, floats: W2L[32][97] at 0, W1L[32][17] behind it
constexpr int kW1L = 32 * kW2LPitch;

// C/D layout of the 32x32 MFMAs: register r of lane half hl holds row rowmap(r, hl)
MRCA_PB_HD int rowmap(int reg, int hl) { return (reg & 3) + 8 * (reg >> 2) + 4 * hl; }

// ---- X: the scan
MRCA_PB_HD int x_off(int row, int ci) { return kXOff + row * kXRowBytes + 2 * ci; }
// where the 4 values x[0..2][i], 0 of input position i go (an 8-byte row)
MRCA_PB_HD int x_stage_off(int i) { return kXOff + (i + 1) * kXRowBytes; }
// conv1 B operand of MFMA mf for output position p: the lane's 16 (mf 0) or 8 (mf 1, hl = 0) bytes
MRCA_PB_HD int conv1_b_off(int mf, int p, int hl) { return mf == 0 ? x_off(2 * p + 2 * hl, 0) : x_off(2 * p + 4, 0); }
// (ci, tap) of element j of the A / B fragments of MFMA mf, lane half hl; ci < 0: a zero element
MRCA_PB_HD int conv1_ci(int mf, int hl, int j) {
    if (mf == 0) return (j & 3) < 3 ? (j & 3) : -1;
    return (hl == 0 && j < 3) ? j : -1;
}
MRCA_PB_HD int conv1_tap(int mf, int hl, int j) { return mf == 0 ? 2 * hl + (j >> 2) : 4; }

// ---- H: relu(conv1)
// the 8-byte row of channels rowmap(4g, hl) .. + 3 at position p (p < 255)
MRCA_PB_HD int h1_store_off(int p, int g, int hl) { return (p + 1) * kHRowBytes + 2 * rowmap(4 * g, hl); }
// conv2 A operand of step s for output position l: 16 bytes = channels 16 (s & 1) + 8 hl .. + 7 of h1 position 2l + tap - 1
MRCA_PB_HD int conv2_a_off(int s, int l, int hl) { return (2 * l + (s >> 1)) * kHRowBytes + 2 * (16 * (s & 1) + 8 * hl); }
MRCA_PB_HD int conv2_ci(int s, int hl, int j) { return 16 * (s & 1) + 8 * hl + j; }
MRCA_PB_HD int conv2_tap(int s) { return s >> 1; }

// ---- O: the output transposition
// the 8-byte run of positions 32 T + rowmap(4g, hl) .. + 3 of channel c
MRCA_PB_HD int out_store_off(int c, int T, int g, int hl) { return kOOff + 2 * (c * kOPitch + 32 * T + rowmap(4 * g, hl)); }
// the 16-byte read q (q < 8) of a lane: channel 4q + lane / 16, positions 8 (lane % 16) .. + 7; feat_elem is where it goes
// in the (robot, tower)'s row of 4096 bf16
MRCA_PB_HD int out_load_off(int q, int lane) { return kOOff + 2 * ((4 * q + (lane >> 4)) * kOPitch + 8 * (lane & 15)); }
MRCA_PB_HD int out_feat_elem(int q, int lane) { return (4 * q + (lane >> 4)) * kL2 + 8 * (lane & 15); }

// conv1 tile t writes H bytes [h_lo(t), h_hi(t)); tile t reads X bytes from x_lo(t) on
MRCA_PB_HD int conv1_h_hi(int t) { return (32 * t + 33) * kHRowBytes; }
MRCA_PB_HD int conv1_x_lo(int t) { return x_off(64 * t, 0); }
constexpr bool x_alias_ok() {
    for (int t = 0; t + 1 < 8; ++t)
        if (conv1_h_hi(t) > conv1_x_lo(t + 1)) return false;
    return true;
}
static_assert(x_alias_ok(), "a conv1 tile overwrites scan rows a later tile reads");
static_assert(kXOff + kXRows * kXRowBytes <= (kHRows - 1) * kHRowBytes, "X stays below H's right padding row");
static_assert(kOOff >= kHRowBytes && kOOff + 2 * kCh * kOPitch <= kXOff, "O stays between H[0] and X");
static_assert(kXOff % 16 == 0 && kOOff % 16 == 0 && (2 * kOPitch) % 16 == 0, "16-byte operand and output rows");
static_assert((kW1L + 32 * kW1LPitch) * 4 <= kWaveBytes, "the weight staging fits the image");

}  // namespace mrca_pbf16
