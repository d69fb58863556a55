"""numpy restatement of the compaction plan of the pair-compacted convolution engine (csrc/conv_pairs_plan.h,
csrc/sparse_conv_pairs.hip), for the tests: per tile of TM output rows and per offset k, the tile's rows whose mask has bit k, in
ascending row order, cut into blocks of SLOTS slots -- and the count of 32-row MFMA blocks this plan and the union walk issue.

The masks are one uint32 word per output row of a table, in the row order the kernel sees (tests/featnet_ref.neighbour_masks over
the levels in that order).  tests/test_conv_pairs_cpu.py pins TM / SLOTS / tile_cols / blocks against the header."""
import numpy as np

TM, SLOTS, THREADS = 128, 32, 256
UNION_TILES = {64: 64, 32: 128}         # the union engine's tile height by tile width (featnet.hip: 64 x 64, else 128 x 32)


def tile_cols(cout):
    """output channels per workgroup (cp_tile_cols)"""
    return 64 if cout % 64 == 0 else 32


def blocks(p):
    """32-slot blocks issued for an offset with p active rows in the tile (cp_blocks)"""
    return (np.asarray(p) + SLOTS - 1) // SLOTS


def bits(mask):
    """[rows] uint32 -> bool [rows, 27]"""
    return ((np.asarray(mask, dtype=np.uint32)[:, None] >> np.arange(27, dtype=np.uint32)) & np.uint32(1)).astype(bool)


def active_counts(mask, tm=TM):
    """P [tiles, 27]: the rows of every tile of tm rows that are active at offset k"""
    b = bits(mask)
    pad = (-len(b)) % tm
    b = np.concatenate([b, np.zeros((pad, 27), bool)])
    return b.reshape(-1, tm, 27).sum(axis=1)


def plan(mask, tm=TM):
    """[tile][k] -> list of blocks, each the tile-local rows of its slots (ascending; the last block may be short)"""
    b = bits(mask)
    out = []
    for m0 in range(0, len(b), tm):
        tile = []
        for k in range(27):
            rows = np.nonzero(b[m0:m0 + tm, k])[0]
            tile.append([rows[s:s + SLOTS] for s in range(0, len(rows), SLOTS)])
        out.append(tile)
    return out


def pairs_blocks(mask, tm=TM):
    """32-slot blocks the pairs engine issues over one table (per 32-column strip and 32-channel slice)"""
    return int(blocks(active_counts(mask, tm)).sum())


def union_blocks(mask, th):
    """32-row blocks the union engine issues with tiles of th rows: th / 32 for every offset some row of the tile uses"""
    return int((active_counts(mask, th) > 0).sum()) * (th // 32)


def useful_blocks(mask):
    """(row, offset) pairs / 32: the blocks a perfect packing would issue"""
    return bits(mask).sum() / SLOTS
