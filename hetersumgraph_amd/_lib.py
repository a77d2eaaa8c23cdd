"""ctypes binding of libhsg.so (the C ABI declared in include/hsg*.h).

The library is built in-tree (``python -m hetersumgraph_amd.build`` or
``__graft_entry__.build()``).  There is deliberately no fallback: if the shared
object is missing or a call fails, a ``RuntimeError`` is raised.

``ABI`` is the one registry of entry points: header file name -> {function name:
argtypes}; ``RESTYPE`` names the few functions that do not return ``int``.  ``load()``
binds from it and nothing else.  The tables are written out (nothing is parsed at
import time, so the package loads a library without include/ beside it) and
tests/test_abi_conformance.py holds them against the headers' declarations, parameter
by parameter.
"""
from __future__ import annotations

import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HSG_LIB_PATH") or os.path.join(_HERE, "libhsg.so")   # override: dev A/B builds

HSG_EINVAL = 1001
HSG_TAU_TABLE = 0
HSG_TAU_PER_EDGE = 1

HSG_EPI_STORE = 0
HSG_EPI_RELU_BWD = 1
HSG_EPI_ADD = 2
HSG_EPI_ADD_ELUG = 3
HSG_IO_A_BF16 = 1
HSG_IO_C_BF16 = 2
HSG_IO_AUX_BF16 = 4


class HsgRel(ctypes.Structure):
    """Mirror of ``struct hsg_rel`` (include/hsg.h)."""

    _fields_ = [("n_src", ctypes.c_int32), ("n_dst", ctypes.c_int32), ("n_edges", ctypes.c_int32),
                ("indptr", ctypes.c_void_p), ("src", ctypes.c_void_p), ("tf", ctypes.c_void_p),
                ("phantom", ctypes.c_void_p), ("cindptr", ctypes.c_void_p),
                ("cdst", ctypes.c_void_p), ("cperm", ctypes.c_void_p),
                ("n_dwork", ctypes.c_int32), ("n_swork", ctypes.c_int32),
                ("dwork", ctypes.c_void_p), ("swork", ctypes.c_void_p)]


class HsgMtTensor(ctypes.Structure):
    """Mirror of ``struct hsg_mt_tensor`` (include/hsg_train.h)."""

    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("n", ctypes.c_int64)]


class HsgResRel(ctypes.Structure):
    """Mirror of ``struct hsg_res_rel`` (include/hsg_resident.h)."""

    _fields_ = [(k, ctypes.c_void_p) for k in ("indptr", "src", "tf", "eid", "phantom", "cindptr", "cdst", "cperm",
                                               "src_nodes", "dst_nodes")]


class HsgResStore(ctypes.Structure):
    """Mirror of ``struct hsg_res_store`` (include/hsg_resident.h)."""

    _fields_ = [("n_docs", ctypes.c_int64), ("starts", ctypes.c_void_p), ("bases", ctypes.c_void_p),
                ("sent_len", ctypes.c_int32), ("label_len", ctypes.c_int32),
                ("unit", ctypes.c_void_p), ("ndtype", ctypes.c_void_p), ("id", ctypes.c_void_p),
                ("sent_rank", ctypes.c_void_p), ("words", ctypes.c_void_p), ("label", ctypes.c_void_p),
                ("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("tffrac", ctypes.c_void_p),
                ("edtype", ctypes.c_void_p), ("rel", HsgResRel * 2)]


class HsgResHdsgCols(ctypes.Structure):
    """Mirror of ``struct hsg_res_hdsg_cols`` (include/hsg_resident_hdsg.h)."""

    _fields_ = [(k, ctypes.c_void_p) for k in ("dstart", "pstart", "pair_s", "pair_d", "doc_sent", "sent_doc",
                                               "sent_super", "doc_super", "sent_ptr", "sent_row", "sup_list",
                                               "inv_cnt", "doc_ptr", "doc_row", "sup_code", "sup_sent", "sup_ptr")]


class HsgResEvalCols(ctypes.Structure):
    """Mirror of ``struct hsg_res_eval_cols`` (include/hsg_resident_eval.h)."""

    _fields_ = [(k, ctypes.c_void_p) for k in ("wstart", "wend", "wid")]


# count families of the resident store (include/hsg_resident.h); q = 0 (W2S), 1 (S2W)
HSG_RES_NODE, HSG_RES_EDGE, HSG_RES_SENT, HSG_RES_NFAM = 0, 1, 2, 9
HSG_RES_SRC = lambda q: 3 + 3 * q
HSG_RES_DST = lambda q: 4 + 3 * q
HSG_RES_TYP = lambda q: 5 + 3 * q

_lib = None

_P = ctypes.c_void_p
_I = ctypes.c_int
_F = ctypes.c_float
_L = ctypes.c_long
_L64 = ctypes.c_int64
_RELP = ctypes.POINTER(HsgRel)
_MTP = ctypes.POINTER(HsgMtTensor)
_RESP = ctypes.POINTER(HsgResStore)

ABI = {}
ABI["hsg.h"] = {
    "hsg_gat_fwd": [_RELP, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "hsg_gat_bwd_dst": [_RELP, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "hsg_gat_bwd_blocks": [_RELP],
    "hsg_gat_bwd_src": [_RELP, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "hsg_gat_bwd_src_blocks": [_RELP],
    "hsg_attn_params_fwd": [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P],
    "hsg_attn_params_fwd_pair": [_I, _I, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _I, _P, _P],
    "hsg_attn_params_fwd_pair_seed": [_I, _I, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P],
    "hsg_attn_params_finish_pair": [_I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I,
                                    _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P],
    "hsg_attn_params_bwd": [_I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P],
    "hsg_attn_params_bwd_workspace_floats": [_I, _I],
    "hsg_attn_params_stage": [_I, _I, _I, _P, _I, _P, _P, _I, _P],
    "hsg_attn_params_finish": [_I, _I, _I] + [_P] * 9 + [_I, _P],
    "hsg_attn_src_logits": [_I, _I, _I, _P, _P, _P, _P],
    "hsg_version": [],
    "hsg_kclock_arm": [_P, _P, _P],
    "hsg_kclock_pending": [],
    "hsg_seed_advance": [_P, _P, _P],
    "hsg_gat_bwd_dst_noh_supported": [_RELP, _I, _I],
    "hsg_gat_bwd_dst_noh": [_RELP, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "hsg_gemm_f32": [_I, _I, _I, _P, _I, _I, _P, _I, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P, _P, _P],
    "hsg_gemm_bf16": [_I, _I, _I, _P, _I, _I, _P, _I, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P, _P, _P],
    "hsg_gemm_f32_mfma": [_I, _I, _I, _P, _I, _I, _P, _I, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P, _P, _P],
    "hsg_gemm_row_tiles": [_I, _I, _I, _I],
    "hsg_ffn_colsums": [_I, _I, _P, _P, _I, _I, _P, _P, _P, _P, _I, _P],
    "hsg_gemm_workspace_floats": [_I, _I, _I, _I],
    "hsg_gemm_auto_splits": [_I, _I, _I],
    "hsg_ln_bwd_blocks": [_I],
    "hsg_dropmask_words": [_I, _I, _I],
    "hsg_dropmask_scale": [_F],
    "hsg_dropmask": [_I, _I, _I, _F, _P, ctypes.c_uint32, _P, _P],
    "hsg_hproj_fwd": [_I, _I, _I, _I, _P, _I, _P, _P, _F, _P, _I, _P],
    "hsg_hproj_fwd_logits_supported": [_I, _I],
    "hsg_hproj_fwd_logits": [_I, _I, _I, _I, _P, _I, _P, _P, _F, _P, _I, _P, _P, _P],
    "hsg_hproj_wt": [_I, _I, _I, _P, _P, _P],
    "hsg_hproj_fwd_t8_supported": [_I, _I, _I],
    "hsg_hproj_fwd_t8": [_I, _I, _I, _P, _I, _P, _P, _F, _P, _I, _P, _P, _P],
    "hsg_hproj_fwd_mf_supported": [_I, _I, _I],
    "hsg_hproj_fwd_mf": [_I, _I, _I, _P, _I, _P, _I, _I, _P, _F, _P, _I, _P, _P, _P],
    "hsg_hproj_dx": [_I, _I, _I, _I, _P, _I, _P, _P, _F, _P, _I, _I, _P],
    "hsg_hproj_dw_chunks": [_I, _I, _I, _I],
    "hsg_hproj_bwd": [_I, _I, _I, _I, _P, _I, _P, _P, _I, _P, _F, _P, _I, _I, _P, _P],
    "hsg_hproj_dw": [_I, _I, _I, _I, _P, _I, _P, _I, _P, _F, _P, _P, _I, _P],
    "hsg_rel_build_workspace_bytes": [_I, _I],
    "hsg_rel_build": [_F, _F, _I, _I] + [_P] * 17 + [ctypes.c_size_t, _P],
    "hsg_cnn_taps": [],
    "hsg_cnn_gather": [_I, _I, _I, _P, _P, _P, _P, ctypes.c_long, _P, _P],
    "hsg_cnn_pool": [_I, _I, _P, _P, _I, _P, _P, _P, _P],
    "hsg_cnn_pool_bwd": [_I, _P, _P, _P, _P, _P, _I, _P],
    "hsg_ln_fwd": [_I, _I, _P, _P, _P, _P, _F, _F, _P, ctypes.c_uint32, _P, _P, _P, _P],
    "hsg_ffn_small_supported": [_I, _I],
    "hsg_ffn_small_bwd_blocks": [_I],
    "hsg_ffn_small_bwd": [_I, _I, _I] + [_P] * 9 + [_F, _P, ctypes.c_uint32] + [_P] * 6,
    "hsg_ffn_small_bwd_gate": [_I, _I, _I] + [_P] * 9 + [_F, _P, ctypes.c_uint32] + [_P] * 9,
    "hsg_ffn_small_fwd": [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _F, _F, _P, ctypes.c_uint32, _P, _P, _P, _P, _P,
                          _P],
    "hsg_ln_bwd": [_I, _I, _P, _P, _P, _P, _P, _P, _F, _P, ctypes.c_uint32, _P, _P, _P, _P],
    "hsg_wsplit_dims": [_I, _I, _P, _P],
    "hsg_dropmask_multi": [_I, _P, _P, _P, _P, _P, _P, _P, _P],
    "hsg_dropmask_multi_wt": [_I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P],
    "hsg_step_prologue": [_I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P],
    "hsg_gemm_f32_slabs": [_I, _I, _I, _P, _I, _I, _P, _I, _I, _I, _P, _P],
    "hsg_gemm_bf16_slabs": [_I, _I, _I, _P, _I, _I, _P, _I, _I, _I, _P, _P],
    "hsg_gemm_dw_slabs": [_I, _P, _P, _I, _P, _P, _P, _P, _I, _I, _P, _P],
    "hsg_gemm_dw_tiles": [_I, _I],
    "hsg_gemm_psw_row_tiles": [_I, _I, _I, _I],
    "hsg_gemm_psw_ln": [_I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _F, _F, _P, ctypes.c_uint32, _P, _P, _P, _I, _P],
    "hsg_slab_reduce": [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "hsg_wsplit": [_I, _P, _P, _P, _P, _P, _P, _P],
    "hsg_gemm_f32_psw": [_I, _I, _I, _P, _I, _P, _P, _I, _P, _P, _I, _I, _I, _P, _P],
    "hsg_gemm_f32_psw_route": [_I, _I, _I],
    "hsg_gemm_f32_psw_plan": [_I, _I, _I, _P, _I, _P, _P, _I, _P, _P, _I, _I, _I, _P, _I, _P],
    "hsg_gemm_f32_psw_elug": [_I, _I, _I, _P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _I, _P],
    "hsg_gemm_bf16_psw": [_I, _I, _I, _P, _I, _P, _P, _I, _P, _P, _I, _I, _I, _P, _P],
    "hsg_gat_bwd_dst_g": [_RELP, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "hsg_gat_bwd_src_g_supported": [_RELP, _I, _I],
    "hsg_gat_bwd_src_g_blocks": [_RELP, _I, _I],
    "hsg_gat_bwd_src_g": [_RELP, _I, _I, _F, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P],
    "hsg_gemm_psw_elug_rho": [_I, _I, _I, _P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _P, _I, _I, _P],
    "hsg_gemm_bf16_psw_io": [_I, _I, _I, _P, _I, _P, _P, _I, _P, _P, _I, _I, _I, _P, _I, _P],
    "hsg_gemm_bf16_psw_elug_rho_a16": [_I, _I, _I, _P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _P, _I, _I, _P],
    "hsg_gemm_psw_elug_rho_gw": [_I, _I, _I, _I, _I],
    "hsg_ln_bwd_dy16": [_I, _I, _P, _P, _I, _P, _P, _P, _P, _F, _P, ctypes.c_uint32, _P, _I, _P, _P, _P],
    "hsg_ln_fwd_y16": [_I, _I, _P, _P, _P, _P, _F, _F, _P, ctypes.c_uint32, _P, _P, _P, _P],
    "hsg_gat_bwd_src_g_io": [_RELP, _I, _I, _F, _P, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P],
    "hsg_gemm_dw_slabs_io": [_I, _P, _P, _I, _P, _P, _P, _P, _P, _I, _P, _P],
    "hsg_rel_work": [_I, _P, _I, _I, _P, _I, _P, _P],
    "hsg_gat_fwd_ws_floats": [_RELP, _I, _I],
    "hsg_gat_fwd_ws": [_RELP, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "hsg_gat_fwd_ws16": [_RELP, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P],
    "hsg_gemm_bf16_psw_elug_rho_x16": [_I, _I, _I, _P, _I, _P, _P, _I, _P, _P, _I, _I, _P, _P, _I, _P, _I, _I, _P],
    "hsg_ln_fwd_x16": [_I, _I, _P, _P, _I, _P, _P, _F, _F, _P, ctypes.c_uint32, _P, _P, _P, _P],
    "hsg_ln_bwd_x16": [_I, _I, _P, _P, _P, _I, _P, _P, _P, _F, _P, ctypes.c_uint32, _P, _I, _P, _P, _P],
    "hsg_lstm_supported": [_I, _I],
    "hsg_lstm_fwd": [_I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P, _P, _F, _P, ctypes.c_uint32, _P, _I, _P],
    "hsg_lstm_bwd": [_I, _I, _I, _I, _P, _P, _I, _P, _P, _P, _F, _P, ctypes.c_uint32, _P, _P],
    "hsg_gat_bwd_src_g_ws_floats": [_RELP, _I, _I],
    "hsg_gat_bwd_src_g_ws": [_RELP, _I, _I, _F, _P, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P],
}
ABI["hsg_train.h"] = {
    "hsg_doc_ce": [_I, _I, _I, _P, _P, _I, ctypes.c_int64, _P, _P, _P, _P, _P, _P, _P],
    "hsg_mt_tensors_per_launch": [],
    "hsg_mt_chunk": [],
    "hsg_mt_blocks": [_MTP, _I],
    "hsg_mt_sqnorm": [_MTP, _I, _P, _P, _P],
    "hsg_mt_adam": [_MTP, _I, _P, _P, _I, _P, _P],
}
ABI["hsg_model.h"] = {
    "hsg_sentfeat_supported": [_I, _I, _I, _I],
    "hsg_sentfeat_rows": [],
    "hsg_sentfeat_fwd": [_I, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P, _I, _P],
    "hsg_sentfeat_bwd": [_I, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _I, _P, _I, _P, _I, _P],
    "hsg_docinit_supported": [_I],
    "hsg_docinit_fwd": [_I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P],
    "hsg_docinit_bwd": [_I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P],
    "hsg_logits_supported": [_I],
    "hsg_logits_fwd": [_I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P],
    "hsg_logits_bwd_blocks": [_I],
    "hsg_logits_bwd": [_I, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P],
}
ABI["hsg_embed.h"] = {
    "hsg_embed_supported": [_I],
    "hsg_embed_rows": [_I, _I, _I, _P, _P, _P, _I, _P],
    "hsg_embed_keys": [_I, _I, _I, _L, _P, _P, _P, _L, _P, _P],
    "hsg_embed_piece_rows": [],
    "hsg_embed_ws_floats": [_L, _I],
    "hsg_embed_grad": [_I, _I, _L, _P, _I, _P, _I, _L, _P, _I, _P, _P, _P],
}
ABI["hsg_eval.h"] = {
    "hsg_eval_select_supported": [_I, _I],
    "hsg_eval_select": [_I, _I, _P, _P, _P, _I, _I, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P],
}
ABI["hsg_eval_words.h"] = {
    "hsg_eval_words_supported": [_I, _I, _I],
    "hsg_eval_select_words": [_I, _I, _P, _P, _P, _I, _I, _I, _P, _P, _I, _P, _I, _P, _P, _P, _P],
}
ABI["hsg_eval_text.h"] = {
    "hsg_eval_text_supported": [_I, _I, _L64],
    "hsg_eval_text_word_bound": [_I, _L64],
    "hsg_eval_text_workspace_bytes": [_I, _I, _L64],
    "hsg_eval_text_words": [_I, _I, _P, _L64, _P, _P, _L64, _P, _P, _P, _P],
}
ABI["hsg_resident.h"] = {
    "hsg_res_supported": [_I, _L64, _L64, _L64],
    "hsg_res_offsets": [_RESP, _I, _P, _P, _P],
    "hsg_res_graph": [_RESP, _I, _P, _P, _L64, _L64] + [_P] * 11,
    "hsg_res_relation": [_RESP, _I, _I, _P, _P, _L64, _L64, _L64] + [_P] * 11,
}
ABI["hsg_resident_model.h"] = {
    "hsg_res_model_supported": [_I, _L64, _L64, _L64],
    "hsg_res_model": [_RESP, _P, _P, _I, _P, _P, _P, _L64, _L64] + [_P] * 9,
}
ABI["hsg_resident_hdsg.h"] = {
    "hsg_res_hdsg_supported": [_I, _L64, _L64, _L64, _L64],
    # cols (const hsg_res_hdsg_cols *) is bound as a plain pointer: pass ctypes.byref(HsgResHdsgCols)
    "hsg_res_hdsg": [_RESP, _P, _I, _P, _P, _P, _P, _L64, _L64, _L64, _L64] + [_P] * 19,
}
ABI["hsg_resident_eval.h"] = {
    "hsg_res_eval_supported": [_I, _L64, _L64],
    # cols (const hsg_res_eval_cols *) is bound as a plain pointer: pass ctypes.byref(HsgResEvalCols)
    "hsg_res_eval": [_RESP, _P, _I, _P, _P, _P, _L64, _L64, _P, _P],
}
ABI["hsg_cnn_tokens.h"] = {
    "hsg_cnn_tok_supported": [_I, _I],
    "hsg_cnn_tok_mark": [_I, _I, _I, _P, _P, _P, _P],
    "hsg_cnn_tok_table": [_I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P],
    "hsg_cnn_tok_pool": [_I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P, _P],
    "hsg_cnn_tok_chunk": [],
    "hsg_cnn_tok_dw_ws_floats": [_I, _I],
    "hsg_cnn_tok_dw": [_I, _I, _I, _I] + [_P] * 8 + [_P, _I, _P, _P],
}
ABI["hsg_cnn_vocab.h"] = {
    "hsg_cnn_vocab_supported": [_I],
    "hsg_cnn_vocab_pool": [_I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _P],
}
ABI["hsg_lstm_train.h"] = {
    "hsg_lstm_train_supported": [_I, _I, _I],
    "hsg_lstm_pack_layer_offset": [_I, _I, _I, _I],
    "hsg_lstm_pack_floats": [_I, _I, _I, _I],
    "hsg_lstm_pack": [_I, _I, _I, _I, _P, _P, _P],
    "hsg_lstm_dw_chunk": [],
    "hsg_lstm_dw_ws_floats": [_I, _I, _I],
    "hsg_lstm_dw": [_I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P],
}
# every function that does not return int
RESTYPE = {"hsg_version": ctypes.c_char_p, "hsg_wsplit_dims": None, "hsg_gemm_workspace_floats": ctypes.c_size_t,
           "hsg_attn_params_bwd_workspace_floats": ctypes.c_size_t,
           "hsg_dropmask_scale": ctypes.c_float,
           "hsg_rel_build_workspace_bytes": ctypes.c_size_t, "hsg_gat_fwd_ws_floats": ctypes.c_size_t,
           "hsg_gat_bwd_src_g_ws_floats": ctypes.c_size_t, "hsg_mt_blocks": ctypes.c_size_t,
           "hsg_embed_ws_floats": ctypes.c_size_t,
           "hsg_eval_text_word_bound": ctypes.c_int64, "hsg_eval_text_workspace_bytes": ctypes.c_size_t,
           "hsg_cnn_tok_dw_ws_floats": ctypes.c_size_t,
           "hsg_lstm_pack_layer_offset": ctypes.c_size_t, "hsg_lstm_pack_floats": ctypes.c_size_t,
           "hsg_lstm_dw_ws_floats": ctypes.c_size_t}


def exports(header):
    """The names one header declares (``exports("hsg_train.h")``), in table order."""
    return tuple(ABI[header])


def load():
    """Load libhsg.so once; raise loudly if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libhsg.so not found at {LIB_PATH}: build it with `python -m hetersumgraph_amd.build` "
            "(hetersumgraph_amd has no CPU fallback for the WSWGAT hot path)")
    lib = ctypes.CDLL(LIB_PATH)
    for sigs in ABI.values():
        for name, args in sigs.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = RESTYPE.get(name, ctypes.c_int)
    _lib = lib
    return lib


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream_of(t: torch.Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


def check(rc: int, what: str):
    if rc != 0:
        kind = "unsupported shape" if rc == HSG_EINVAL else f"hipError {rc}"
        raise RuntimeError(f"{what} failed: {kind}")


def version() -> str:
    return load().hsg_version().decode()


_is_dev = None
_OPTIONS = {}


def is_dev() -> bool:
    """True when the loaded library is the dev build (libhsg_dev.so via HSG_LIB_PATH)."""
    global _is_dev
    if _is_dev is None:
        _is_dev = version().endswith(" dev")
    return _is_dev


def path_option(name: str, default: str) -> str:
    """A Python-side path switch (e.g. ``HSG_FUSED_STACK``): an explicit selection made
    with :func:`path_options` first; the environment variable of the same name only
    when the dev library is loaded (the A/B tools); otherwise the measured default.
    The product path therefore never changes algorithm or precision because of the
    environment (the C library's switches follow the same rule, csrc/hsg_dev.h)."""
    if name in _OPTIONS:
        return _OPTIONS[name]
    if is_dev():
        return os.environ.get(name, default)
    return default


class path_options:
    """``with path_options(HSG_FUSED_STACK="0"): ...`` -- explicit, scoped path
    selections for tests and tools (values are strings, as the environment's)."""

    def __init__(self, **kw):
        self.kw = {k: str(v) for k, v in kw.items()}

    def __enter__(self):
        self.prev = dict(_OPTIONS)
        _OPTIONS.update(self.kw)
        return self

    def __exit__(self, *exc):
        _OPTIONS.clear()
        _OPTIONS.update(self.prev)


class KernelClock:
    """In-step kernel timing for bench.py: while a clock is active (``with
    KernelClock() as clk``), tagged edge launches are timed inside an ordinary
    (eager) training step -- so each kernel runs after the step's real predecessors,
    with the caches they leave.  The two HIP events of a launch are recorded by the
    kernels' own dispatch packets (``hsg_kclock_arm`` -> hipExtLaunchKernel: start at
    the entry point's first kernel, stop at its last), not by event packets around
    them.  Off (the default), the hook costs one global read per launch."""

    def __init__(self):
        self.events = {}

    def __enter__(self):
        global CLOCK
        CLOCK = self
        return self

    def __exit__(self, *exc):
        global CLOCK
        CLOCK = None

    def start(self, tag, device):
        st = torch.cuda.current_stream(device)
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record(st)                   # creates the events; the kernels re-record them
        e1.record(st)
        load().hsg_kclock_arm(st.cuda_stream, e0.cuda_event, e1.cuda_event)
        return (tag, e0, e1)

    def stop(self, token, device):
        tag, e0, e1 = token
        if load().hsg_kclock_pending():
            load().hsg_kclock_arm(None, None, None)
            raise RuntimeError(f"kernel clock {tag}: the launch path did not record the armed events")
        self.events.setdefault(tag, []).append((e0, e1))

    @staticmethod
    def disarm():
        """Drop this thread's armed events (error path: the entry point raised before
        its launches consumed them, so they must not outlive their Event objects)."""
        load().hsg_kclock_arm(None, None, None)

    def durations_ms(self):
        """tag -> list of per-launch durations (ms); synchronises."""
        torch.cuda.synchronize()
        return {t: [a.elapsed_time(b) for a, b in evs] for t, evs in self.events.items()}


CLOCK = None
