// conv_pairs_plan.h -- the tile plan of the pair-compacted convolution engine (sparse_conv_pairs.hip), host and device.
//
// A workgroup owns kCpTM output rows x TN output channels (TN = 64 where C_out allows, else 32).  For every offset k the tile's
// rows that have a neighbour at k -- P_k of them, in ascending row order -- fill slots 0 .. P_k - 1, and the matrix unit is
// fed cp_blocks(P_k) blocks of kCpSlots slots (the last one padded).  kCpTM is a multiple of both tile heights of the union
// engine (64 with TN = 64, 128 with TN = 32), so this plan never issues more 32-row blocks than the union walk does: a union tile
// issues tile height / 32 blocks for an offset that any of its rows uses, and the rows of one union tile fill at most that many
// blocks here.  tests/conv_pairs_ref.py restates the plan, tests/test_conv_pairs_cpu.py pins it against this header.
#pragma once

namespace umereg {

constexpr int kCpTM = 128;          // output rows per workgroup
constexpr int kCpSlots = 32;        // slots per MFMA block (the M of v_mfma_f32_32x32x2_f32 / v_mfma_f32_32x32x16_f16)
constexpr int kCpThreads = 256;

// output channels per workgroup for a layer with `cout` output channels
constexpr int cp_tile_cols(int cout) { return cout % 64 == 0 ? 64 : 32; }
// 32-slot blocks issued for an offset with `p` active rows in the tile
constexpr int cp_blocks(int p) { return (p + kCpSlots - 1) / kCpSlots; }

}  // namespace umereg
