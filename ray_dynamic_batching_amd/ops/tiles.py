"""Tile tables, tile-choice encodings and the candidate lists the tuner ranks.

The kernels take a tile index (gemm_core.h kTileBM / kTileBN, conv.hip
kConvPP*, conv_halo.hip kHalo*).  The tables below are the Python copy of that
geometry: they feed the candidate generators, the CU-time ranking and the
split-K workspace bound, and work on a host without the built extension.
``_ops().tile_tables()`` exports the C++ side; tests/test_tile_tables.py holds
the two equal, field by field."""
from __future__ import annotations

import os

from ._common import _ops
from .diag import _v4_tiles_built

# ---------------------------------------------------------------------------
# Dense GEMM / implicit-GEMM conv tiles (gemm_core.h)
# ---------------------------------------------------------------------------
NUM_TILE_CFGS = 30   # gemm_core.h kTileBM/BN: 0..12 4-wave (GEMM and conv), 13..18 8-wave, 19..25 ping-pong,
                     # 26..28 4-wave VGPR-staged one-block-per-CU tiles (gemm_v4.h; GEMM only, K % 64 == 0),
                     # 29 ping-pong 256x224 (the Llama gate-up N = 28672 = 128 x 224)
NUM_LN_TILE_CFGS = 19  # the deferred-LayerNorm epilogues run on tiles 0..18
NUM_CONV_TILE_CFGS = 13   # gemm_core.h kNumTiles4
FORCE_TILED = 99      # tile_cfg value that bypasses the skinny-M GEMM (M <= 64)
SKINNY_MAX_M = 64
# gemm_core.h kTileBM / kTileBN / kTileNW
_ALL_BM = (128, 64, 128, 64, 128, 192, 256, 128, 128, 64, 128, 256, 128, 256, 128, 256, 256, 128, 256, 256, 256, 128,
           256, 256, 256, 256, 128, 128, 256, 256)
_ALL_BN = (128, 128, 64, 64, 192, 128, 128, 256, 144, 96, 96, 144, 48, 128, 256, 192, 144, 96, 96, 128, 144, 256, 256,
           128, 192, 192, 96, 128, 192, 224)
_ALL_NW = (4,) * 13 + (8,) * 13 + (4,) * 3 + (8,)
_TILE_BM = _ALL_BM[:NUM_CONV_TILE_CFGS]      # the 4-wave tiles (GEMM and conv)
_TILE_BN = _ALL_BN[:NUM_CONV_TILE_CFGS]
STG_TILE_CFGS = (0, 9, 10, 12, 19, 21, 23, 24)   # gemm_core.h kStgTiles
_SWIGLU_TILE_CFGS = tuple(range(26)) + (29,)   # the VGPR-staged tiles (26..28) have no SwiGLU epilogue

# ---------------------------------------------------------------------------
# Encoded tile choices (what the tuner / tile tables store):
#   cfg                  4-wave tile cfg (0..12) of the implicit-GEMM conv kernel
#   cfg | splits << 8    the same tile, split-K over `splits` workgroups per tile
#   CONV_LINEAR | cfg    (1x1 / stride 1) the dense GEMM `linear` on tile cfg (0..25)
#   ... | DEEP           tiles 0, 1, 2, 3, 9, 10 with one block per CU and up to 8 LDS stages
# ---------------------------------------------------------------------------
DEEP = 1 << 12                        # gemm_core.h kDeepFlag: one block per CU, up to 8 LDS stages
_DEEP_TILES = (0, 1, 2, 3, 9, 10, 6, 7)
_DEEP_BIG = (6, 7)                    # 256x128 / 128x256: one block per CU at any grid size
_DEEP_MAX_BLOCKS = 320                # DEEP candidates only where the grid is ~one block per CU
CONV_LINEAR = 1 << 16
#   CONV_PP | v [| splits << 8]   (R x S / strided convs, C % BK == 0, with bias) the
#                        8-wave ping-pong kernel with the im2col operand, tile v (conv.hip)
CONV_PP = 1 << 17
_CONV_PP_BM = (256, 128, 256, 256, 128)          # conv.hip kConvPPBM / BN / BK
_CONV_PP_BN = (128, 256, 128, 64, 128)
_CONV_PP_BK = (64, 64, 32, 64, 32)
#   CONV_HALO | v        (3x3, stride 1, pad 1, C % 64 == 0, with bias) the halo-tile kernel,
#                        tile v (conv_halo.hip): one LDS patch feeds all 9 taps
CONV_HALO = 1 << 18
_CONV_HALO_BM = (256, 112, 112, 64, 224, 224, 64, 128, 256, 256, 64, 64)    # conv_halo.hip kHaloBM / kHaloBN
_CONV_HALO_BN = (64, 64, 64, 64, 64, 128, 64, 32, 64, 64, 128, 64)
_CONV_HALO_RW = (6, 7, 8)          # persistent resident-weight tiles: no residual, ReLU / none (stride 1)
_CONV_HALO_SK = (2, 3, 4, 5, 9, 10, 11)   # two-patch-buffer streamed tiles: split-K over the 64-channel blocks

# ---------------------------------------------------------------------------
# Split-K
# ---------------------------------------------------------------------------
SPLITK_HEADER = 65536                 # gemm_core.h kSplitKHeader (tile arrival counters)
SPLITK_WS_BYTES = 40 << 20            # one forward's split-K workspace (ops.splitk_workspace)
_SPLITS = (2, 3, 4, 6, 8)
_PP_SPLITK_TILES = (19, 21)           # ping-pong tiles with a split-K instantiation (BK 64, gemm_core.h pp_splitk_tile)

# ---------------------------------------------------------------------------
# Candidate switches
# ---------------------------------------------------------------------------
# RDB_CONV1X1_GEMM=0 keeps 1x1 convolutions off the dense `linear` tiles
_CONV1X1_GEMM = os.environ.get("RDB_CONV1X1_GEMM", "1") != "0"
# RDB_CONV_SPLITK=0: no split-K candidates
_CONV_SPLITK = os.environ.get("RDB_CONV_SPLITK", "1") != "0"
# RDB_GEMM_SPLITK=0: no split-K candidates for the dense GEMM (linear)
_GEMM_SPLITK = os.environ.get("RDB_GEMM_SPLITK", "1") != "0"
# RDB_GEMM_DEEP=0: no DEEP (one block per CU, many LDS stages) tile candidates
_GEMM_DEEP = os.environ.get("RDB_GEMM_DEEP", "1") != "0"
# RDB_CONV_PP=0: no ping-pong conv candidates
_CONV_PP = os.environ.get("RDB_CONV_PP", "1") != "0"
# RDB_CONV_HALO=0: no halo-tile conv candidates
_CONV_HALO = os.environ.get("RDB_CONV_HALO", "1") != "0"


def splits_of(c: int) -> int:
    """Split-K factor of an encoded tile choice (0 / 1: not split).  The factor is
    the 4-bit field at bit 8 (gemm_core.h decodes ``(cfg >> 8) & 15``): the DEEP
    flag (bit 12), CONV_LINEAR (bit 16) and CONV_PP (bit 17) are not part of it;
    a CONV_LINEAR choice is never split."""
    return 0 if c < 0 or (c & CONV_LINEAR) else (c >> 8) & 15


def _blocks_per_cu(t: int) -> int:
    """gemm_core.h tile_blocks_per_cu (CU-time estimates of the tuner)."""
    if t == 23:
        return 2
    if t >= 19:                     # ping-pong and VGPR-staged tiles: one block per CU
        return 1
    q = 8 * _ALL_NW[t]
    bnp = -(-_ALL_BN[t] // q) * q
    return max(1, min(8 // _ALL_NW[t], 163840 // (2 * (_ALL_BM[t] + bnp) * 64 * 2)))


def _key_mn(key: tuple):
    """(M, N) of the output a tuning key's launches write: dense GEMM keys carry
    them, conv keys give N*P*Q output pixels x K channels; None otherwise."""
    if key[0] == "gemm":
        return key[2], key[3]
    if key[0] == "conv":
        N, H, W, C, K, R, S, stride, pad = key[1:10]
        P, Q = (key[13], key[14]) if len(key) >= 15 else ((H + 2 * pad - R) // stride + 1,
                                                           (W + 2 * pad - S) // stride + 1)
        return N * P * Q, K
    return None


def _cu_share(c: int, M: int, N: int, cus: int = 256) -> float:
    """Share of the GPU's CUs a GEMM launch with tile choice ``c`` holds (split-K
    multiplies the blocks, DEEP holds a whole CU per block)."""
    t = c & 255
    if c >= 0 and c & CONV_HALO:
        if not 0 <= t < len(_CONV_HALO_BM):
            return 1.0
        return min(1.0, -(-M // _CONV_HALO_BM[t]) * -(-N // _CONV_HALO_BN[t]) * max(1, (c >> 8) & 15) / cus)
    if c >= 0 and c & CONV_PP:
        if not 0 <= t < len(_CONV_PP_BM):
            return 1.0
        blocks = -(-M // _CONV_PP_BM[t]) * -(-N // _CONV_PP_BN[t]) * max(1, (c >> 8) & 15)
        return min(1.0, blocks / (cus * (2 if _CONV_PP_BK[t] == 32 else 1)))   # BK 32 tiles: 2 blocks / CU
    if not 0 <= t < len(_ALL_BM):
        return 1.0
    blocks = -(-M // _ALL_BM[t]) * -(-N // _ALL_BN[t]) * max(1, (c >> 8) & 15)
    per_cu = 1 if c & DEEP else _blocks_per_cu(t)
    return min(1.0, blocks / (cus * per_cu))


def _gemm_candidates(M: int, N: int, K: int, splitk: bool = False):
    """Dense GEMM tile choices: every tile cfg, plus the DEEP variants of the
    4-wave tiles whose grid is about one block per CU (``DEEP`` flag), plus
    (``splitk``) split-K variants of the 4-wave tiles and the BK-64 ping-pong
    tiles 19 / 21 where the tile grid leaves CUs idle and each split keeps >= 8 K
    steps (long-K GEMMs of small M: the Llama prefill's down projection at 128
    tokens is 128 blocks x 224 K steps; at 1024 tokens 128 ping-pong tiles)."""
    # VGPR-staged tiles 26..28: K % 64 == 0, and only in the experimental build (they tied
    # or lost every engine A/B, profiles/ab_r5_v4_bert.json)
    v4 = K % 64 == 0 and _v4_tiles_built()
    cands = [c for c in range(NUM_TILE_CFGS) if not 26 <= c <= 28 or v4]
    if _GEMM_DEEP and K >= 256:
        cands += [c | DEEP for c in _DEEP_TILES
                  if c in _DEEP_BIG or -(-M // _TILE_BM[c]) * -(-N // _TILE_BN[c]) <= _DEEP_MAX_BLOCKS]
    if splitk and _GEMM_SPLITK:
        nk = -(-K // 64)
        for c in list(range(NUM_CONV_TILE_CFGS)) + list(_PP_SPLITK_TILES):
            tiles = -(-M // _ALL_BM[c]) * -(-N // _ALL_BN[c])
            if tiles >= 256:
                continue
            for sp in _SPLITS:
                kper = -(-nk // sp)
                eff = -(-nk // kper)
                if eff < 2 or kper < 8 or tiles * eff > 1024:
                    continue
                if SPLITK_HEADER + tiles * eff * _ALL_BM[c] * _ALL_BN[c] * 4 > SPLITK_WS_BYTES:
                    continue
                cands.append(c | (sp << 8))
    return cands


def _conv_pp_candidates(M: int, K_out: int, Kg: int, C: int):
    """Ping-pong conv tiles (CONV_PP) for an im2col conv: every tile whose BK
    divides C, split-K where the grid is under ~one block per CU."""
    out = []
    if K_out % 8:
        return out
    for v in range(len(_CONV_PP_BM)):
        bm, bn, bk = _CONV_PP_BM[v], _CONV_PP_BN[v], _CONV_PP_BK[v]
        if C % bk:
            continue
        tiles = -(-M // bm) * -(-K_out // bn)
        out.append(CONV_PP | v)
        if not _CONV_SPLITK or tiles >= 256:
            continue
        nk = Kg // bk
        for sp in _SPLITS + (12,):
            kper = -(-nk // sp)
            eff = -(-nk // kper)
            if eff < 2 or kper < 3 or tiles * eff > 1024:
                continue
            if SPLITK_HEADER + tiles * eff * bm * bn * 4 > SPLITK_WS_BYTES:
                continue
            out.append(CONV_PP | v | (sp << 8))
    return out


def conv_halo_candidates(N: int, H: int, W: int, C: int, K: int, R: int, S: int, stride: int, pad: int, P: int,
                         Q: int, has_bias: bool, has_res: bool = False, act: str = "relu"):
    """Halo-tile 3x3 tiles (CONV_HALO | v [| splits << 8]) whose rows fit the image
    (conv_halo.hip ``conv_halo_tiles_s``): 3x3 convs with pad 1, stride 1 or 2, the full
    output, a bias; the one-patch-buffer tiles only for a single 64-channel block
    (C == 64), the resident-weight tiles only at stride 1; split-K where the tile
    grid leaves CUs idle."""
    if not (_CONV_HALO and has_bias and R == 3 and S == 3 and stride in (1, 2) and pad == 1
            and (P, Q) == ((H - 1) // stride + 1, (W - 1) // stride + 1) and C % 64 == 0 and K % 8 == 0):
        return []
    rw_ok = not has_res and act in ("relu", "none")
    out = []
    for v in range(len(_CONV_HALO_BM)):
        tiles = _ops().conv_halo_tiles_s(v, N, H, W, C, K, stride)
        if tiles <= 0 or (v in _CONV_HALO_RW and not rw_ok):
            continue
        out.append(CONV_HALO | v)
        if v not in _CONV_HALO_SK or not _CONV_SPLITK or tiles >= 256:
            continue
        # split-K where the tile grid leaves CUs idle (stages 3 / 4 of ResNet-50 at small batch)
        ncb = C // 64
        for sp in (2, 3, 4, 8):
            cpb = -(-ncb // sp)
            eff = -(-ncb // cpb)
            if eff < 2 or eff != sp or tiles * eff > 1024:
                continue
            if _ops().conv_halo_ws_bytes(v, N, H, W, C, K, sp, stride) > SPLITK_WS_BYTES:
                continue
            out.append(CONV_HALO | v | (sp << 8))
    return out


def _conv_candidates(M: int, K_out: int, Kg: int, one_by_one: bool, C: int = 0, has_bias: bool = False):
    """Tile choices for a conv of output [M, K_out] over a Kg-long reduction:
    every 4-wave tile; split-K where the tile grid leaves CUs idle (< 2 blocks
    per CU) and each split keeps >= 4 K-steps; the dense GEMM tiles for 1x1;
    the ping-pong conv tiles for the im2col convs (with a bias)."""
    cands = list(range(NUM_CONV_TILE_CFGS))
    nk = -(-Kg // 64)

    def tiles_of(c):
        return -(-M // _TILE_BM[c]) * -(-K_out // _TILE_BN[c])

    if _GEMM_DEEP:
        cands += [c | DEEP for c in _DEEP_TILES if (c in _DEEP_BIG or tiles_of(c) <= _DEEP_MAX_BLOCKS) and nk >= 4]
    if _CONV_SPLITK:
        for c in range(NUM_CONV_TILE_CFGS):
            tiles = tiles_of(c)
            if tiles >= 512:
                continue
            for sp in _SPLITS:
                kper = -(-nk // sp)
                eff = -(-nk // kper)
                if eff < 2 or kper < 4 or tiles * eff > 2048:
                    continue
                if SPLITK_HEADER + tiles * eff * _TILE_BM[c] * _TILE_BN[c] * 4 > SPLITK_WS_BYTES:
                    continue
                cands.append(c | (sp << 8))
                if _GEMM_DEEP and c in _DEEP_TILES and tiles * eff <= _DEEP_MAX_BLOCKS and kper >= 4:
                    cands.append(c | (sp << 8) | DEEP)
    if one_by_one and _CONV1X1_GEMM and K_out % 8 == 0:
        cands += [CONV_LINEAR | c for c in _gemm_candidates(M, K_out, Kg)]
    if not one_by_one and has_bias and _CONV_PP:
        cands += _conv_pp_candidates(M, K_out, Kg, C)
    return cands
