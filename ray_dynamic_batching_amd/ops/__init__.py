"""Python wrappers of the gfx950 kernels, plus plain-PyTorch fp32 references.

Every wrapper validates shapes / dtypes / strides / alignment on the host
before launching (a mis-shaped launch on the GPU can take the whole node down),
allocates its output with the torch caching allocator and launches on
``torch.cuda.current_stream()`` -- so the calls are capturable into hipGraphs.

The ``*_ref`` functions are the numerics references used by the tests and the
eager baseline path of the models (``backend="torch"``); each stays beside the
wrapper it anchors.

One concern per module: ``tiles`` (tile tables, encodings, candidate lists),
``tuning`` (the per-shape autotuner), ``splitk`` (split-K workspaces), ``gemm``,
``gemm_ln``, ``norm``, ``fp8``, ``attn``, ``conv``, ``diag``.  This file only
re-exports them as ``ops.NAME``.  Module state that is rebound (not mutated)
is read through its owner: ``tuning._KEY_LOG``, ``tuning._tune_graph_broken``,
``diag._V4_BUILT``.
"""
from __future__ import annotations

from . import attn, conv, diag, fp8, gemm, gemm_ln, norm, splitk, tiles, tuning  # noqa: F401
from ._common import (ACT_CODE, DTYPE_CODE, _act_ref, _aligned, _check, _ops, _ptr, _stream,  # noqa: F401
                      require_gpu_ops)
from .attn import (NUM_QKV_ATTN_CFGS, QKV_ATTN_MAX_S, attention, attention_ref, embed_ln, embed_ln_ref,  # noqa: F401
                   gather_rows, pack_qkv_heads, pack_qkv_vec, qkv_attention, qkv_attention_ref,
                   qkv_attention_supported, rope_, rope_ref, rope_tables, seq_lens, seq_lens_ref, softmax_topk,
                   softmax_topk_packed, softmax_topk_ref)
from .conv import (avgpool_nhwc, avgpool_nhwc_ref, conv2d_nhwc, conv2d_nhwc_ref, dwconv_nhwc,  # noqa: F401
                   dwconv_nhwc_ref, image_to_nhwc, image_to_nhwc_ref, image_to_s2d, image_to_s2d_ref, maxpool_nhwc,
                   maxpool_nhwc_ref, se_scale, se_scale_ref, shuffle_remap, shuffle_remap_ref, stem_s2d_pool,
                   stem_weight_s2d)
from .diag import BlockStamps, _v4_tiles_built, experimental_kernels_built, stamps_built  # noqa: F401
from .fp8 import (FP8_DTYPE, FP8_MAX, _FP8_ACTS, _fp8_quant_f32, _fp8_rows, fp8_num_tiles, linear_fp8,  # noqa: F401
                  linear_fp8_ref, linear_w8a8, quantize_fp8_rows, quantize_fp8_rows_ref, quantize_weight_fp8,
                  rms_norm_fp8, rms_norm_fp8_ref)
from .gemm import linear, linear_ref, linear_streamk, streamk_workspace  # noqa: F401
from .gemm_ln import (LN_LNA, LN_LNR, LN_OUT, LN_SELF, LN_STATS, LN_STG, _LNOUT_ERR, _PSTATS_MAX,  # noqa: F401
                      _lnout_err, _pstats_layout, _stats_ld, fold_ln_weights, linear_ln, linear_ln_ref,
                      linear_ln_staged, linear_residual_ln, linear_residual_ln_ref, linear_rowln,
                      linear_rowln_supported, ln_out_error, pack_rowln_weight)
from .norm import _norm, layer_norm, layer_norm_ref, rms_norm, rms_norm_ref  # noqa: F401
from .splitk import (_cap_ws_local, _priv_ws, _private_splitk_ws, _tune_launcher, _tune_ws,  # noqa: F401
                     capture_splitk_workspace, splitk_workspace)
from .tiles import (CONV_HALO, CONV_LINEAR, CONV_PP, DEEP, FORCE_TILED, NUM_CONV_TILE_CFGS,  # noqa: F401
                    NUM_LN_TILE_CFGS, NUM_TILE_CFGS, SKINNY_MAX_M, SPLITK_HEADER, SPLITK_WS_BYTES, STG_TILE_CFGS,
                    _ALL_BM, _ALL_BN, _ALL_NW, _CONV1X1_GEMM, _CONV_HALO, _CONV_HALO_BM, _CONV_HALO_BN,
                    _CONV_HALO_RW, _CONV_HALO_SK, _CONV_PP, _CONV_PP_BK, _CONV_PP_BM, _CONV_PP_BN, _CONV_SPLITK,
                    _DEEP_BIG, _DEEP_MAX_BLOCKS, _DEEP_TILES, _GEMM_DEEP, _GEMM_SPLITK, _PP_SPLITK_TILES, _SPLITS,
                    _SWIGLU_TILE_CFGS, _TILE_BM, _TILE_BN, _blocks_per_cu, _conv_candidates, _conv_pp_candidates,
                    _cu_share, _gemm_candidates, _key_mn, conv_halo_candidates, splits_of)
from .tuning import (_TUNE, _TUNE_GRAPH, _TUNE_STREAMS, _TUNE_TOP, _key_from_json, _key_json,  # noqa: F401
                     _time_tile_graph, _tune_streams, _tuned_cfg, autotune_enabled, load_tuning,
                     record_tuning_keys, save_tuning, tune_in_context, tuning_table)
