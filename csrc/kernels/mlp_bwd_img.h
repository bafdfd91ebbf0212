// LDS images of the dact2 and X tiles of mlp_bwd4 (mlp_step.hip), filled by LDS-DMA
// (global_load_lds_dwordx4): one wave-instruction writes 1 KiB lane-linearly (lane l's 16 bytes at
// base + 16 l) from a per-lane source address.  An image is therefore a sequence of 1 KiB pieces; what
// a piece holds is chosen by which global 16-byte chunk each lane fetches, padding is possible only
// between pieces.  All offsets are in bf16 elements (a chunk = 8 elements).  Shared by the kernel
// and by the host checker tools/check_mlp_bwd_img.cpp, which proves: every chunk of a tile written
// exactly once and inside its buffer, every reader's elements, every read conflict-free.
//
// dact2 tile (64 rows x 256, global rows verbatim: the forward already swapped the chunk pairs of
// rows with bit 2 set, column ^ 8): piece p = rows p and p + 32, 512 bytes each, pieces 1056 bytes
// apart.  Row r at (r & 31) * 528 + (r >> 5) * 256: a [32][2][256] image of pitch 264 dwords (8 mod
// 64, as the register-staged image's 136).  The two rows of a piece are never read by one
// instruction ((a): a wave's 16 rows; (b) / db1: 8 consecutive rows per 32-lane half), so the 16-byte
// slot of chunk c of row r is (2 r + (c ^ bit 2 of r)) mod 16 for every reader, as before.
//
// X tile (64 rows x K0, contiguous in global memory): piece t = the 1 KiB of rows t * 512 / K0 ..., no
// padding; chunk c of row r at chunk c ^ x_swz(r) of its row.  K0 = 64 (8 chunks per row): x_swz =
// 2 ((r >> 1) & 3), slot (8 (r & 1) + (c ^ x_swz)) mod 16.  K0 = 32 (4 chunks): x_swz = 2 ((r >> 2) & 1),
// slot (4 (r & 3) + (c ^ x_swz)) mod 16.  The 8 rows x 2 chunks of a transposing read's 32-lane half
// and the 16 (row, chunk) pairs of a 16-byte read's lane group then cover the 16 slots once.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HAR_IMG_FN __host__ __device__ constexpr
#else
#define HAR_IMG_FN constexpr
#endif

namespace bwdimg {

constexpr int ROWS = 64;    // rows of a tile
constexpr int H = 256;      // dact2 columns
constexpr int CHUNK = 8;    // elements of a 16-byte chunk
constexpr int PIECE = 512;  // elements one LDS-DMA wave-instruction writes

// ---- dact2 ----
constexpr int D2_PIECES = ROWS * H / PIECE;  // 32
constexpr int D2_PITCH = 2 * H + 16;         // piece pitch
constexpr int D2_ELEMS = D2_PIECES * D2_PITCH;
// LDS offset of piece p (wave-uniform; lane l lands at + 8 l)
HAR_IMG_FN int d2_dst(int p) { return p * D2_PITCH; }
// offset inside the global tile ([64][256]) of the chunk lane l of piece p fetches
HAR_IMG_FN int d2_src(int p, int lane) { return (p + 32 * (lane >> 5)) * H + CHUNK * (lane & 31); }
// first element of tile row r
HAR_IMG_FN int d2_row(int r) { return (r & 31) * D2_PITCH + (r >> 5) * H; }
// The readers' offsets are written flat (a lane term + a wave-uniform term + a compile-time term), so
// that every unrolled read is one lane base register + an immediate; the checker compares them with
// d2_row / x_off.
// (a) 16-byte read of lane (c16, g): row 16 rb + c16 (row block rb < 4), logical columns 32 kc + 8 g .. + 7
HAR_IMG_FN int d2_a_off(int rb, int c16, int kc, int g) {
  return c16 * D2_PITCH + ((8 * g) ^ (8 * ((c16 >> 2) & 1))) + (rb & 1) * (16 * D2_PITCH) + (rb >> 1) * H + kc * 32;
}
// (b) / db1 transposing 8-byte read `hi` (0 / 1) of lane l: row 32 ks + 4 g + (li >> 2) + 16 hi,
// logical columns col0 + 4 (li & 3) .. + 3 (col0 a multiple of 16)
HAR_IMG_FN int d2_b_row(int ks, int lane, int hi) { return 32 * ks + 4 * (lane >> 4) + ((lane & 15) >> 2) + 16 * hi; }
HAR_IMG_FN int d2_b_off(int ks, int col0, int lane, int hi) {
  return (4 * (lane >> 4) + ((lane & 15) >> 2)) * D2_PITCH + ((4 * (lane & 3)) ^ (8 * ((lane >> 4) & 1))) + col0 +
         hi * (16 * D2_PITCH) + ks * H;
}

// ---- X ----
HAR_IMG_FN int x_elems(int K0) { return ROWS * K0; }
HAR_IMG_FN int x_pieces(int K0) { return ROWS * K0 / PIECE; }
HAR_IMG_FN int x_swz(int K0, int r) { return K0 == 64 ? 2 * ((r >> 1) & 3) : 2 * ((r >> 2) & 1); }
// chunk c of row r
HAR_IMG_FN int x_off(int K0, int r, int c) { return r * K0 + CHUNK * (c ^ x_swz(K0, r)); }
HAR_IMG_FN int x_dst(int t) { return t * PIECE; }
// offset inside the global tile ([64][K0], contiguous) of the chunk lane l of piece t fetches: LDS
// chunk 64 t + l is position l % (K0 / 8) of row (64 t + l) / (K0 / 8)
HAR_IMG_FN int x_src(int K0, int t, int lane) {
  const int r = (64 * t + lane) / (K0 / CHUNK), pos = lane % (K0 / CHUNK);
  return r * K0 + CHUNK * (pos ^ x_swz(K0, r));
}
// h1 recompute, 16-byte read of lane (c16, g): row `row`, columns 32 kc + 8 g .. + 7
HAR_IMG_FN int x_h1_off(int K0, int row, int kc, int g) { return x_off(K0, row, 4 * kc + g); }
// (c) transposing 8-byte read `hi` of lane l: row 32 ks + 4 g + (li >> 2) + 16 hi, columns
// 16 f + 4 (li & 3) .. + 3
HAR_IMG_FN int x_c_row(int ks, int lane, int hi) { return 32 * ks + 4 * (lane >> 4) + ((lane & 15) >> 2) + 16 * hi; }
HAR_IMG_FN int x_c_off(int K0, int ks, int f, int lane, int hi) {
  return x_off(K0, x_c_row(ks, lane, hi), 2 * f + ((lane >> 1) & 1)) + 4 * (lane & 1);
}

}  // namespace bwdimg
