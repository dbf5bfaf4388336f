"""ctypes binding of liblgcn.so (C ABI: include/lgcn.h).  Fails loudly when the library is absent."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblgcn.so")

MAX_REL = 16
REL_IDENT, REL_CSR, REL_RANGE, REL_RANGE16 = 0, 1, 2, 3
F_GN1, F_RELU1, F_GEMM2, F_GN2, F_RES, F_RELU2 = 1, 2, 4, 8, 16, 32
MMA_F32, MMA_BF16X3, MMA_BF16, MMA_F16X2 = 0, 1, 2, 3
MMA_NAMES = {"f32": MMA_F32, "bf16x3": MMA_BF16X3, "bf16": MMA_BF16, "f16x2": MMA_F16X2}


class LgcnError(RuntimeError):
    pass


class Rel(C.Structure):
    _fields_ = [("src", C.c_void_p), ("wp", C.c_void_p), ("mode", C.c_int32), ("ridx", C.c_int32)]


class PairsJob(C.Structure):      # lgcn_pairs_job_t
    _fields_ = [
        ("agt_ctrs", C.c_void_p), ("agt_off", C.c_void_p), ("ctx_ctrs", C.c_void_p), ("ctx_off", C.c_void_p),
        ("n_scenes", C.c_int32), ("legacy_offsets", C.c_int32), ("n_agt", C.c_int64), ("n_ctx", C.c_int64),
        ("dist_th", C.c_float), ("pad_", C.c_int32),
        ("hi", C.c_void_p), ("wi", C.c_void_p), ("cap", C.c_int64),
        ("n_pairs", C.c_void_p), ("rowptr", C.c_void_p), ("ws", C.c_void_p),
    ]


class Index(C.Structure):         # lgcn_index_t
    _fields_ = [
        ("idx_local", C.c_void_p), ("n_elem", C.c_int64),
        ("seg_off", C.c_void_p), ("seg_base", C.c_void_p), ("n_seg", C.c_int32), ("n_rel", C.c_int32),
        ("u_off", C.c_int64 * MAX_REL), ("v_off", C.c_int64 * MAX_REL), ("n_edges", C.c_int64 * MAX_REL),
        ("n_nodes", C.c_int64),
        ("rowptr", C.c_void_p), ("col", C.c_void_p), ("cnt", C.c_void_p), ("uv", C.c_void_p),
        ("jobs", C.c_void_p), ("n_jobs", C.c_int32), ("pad_", C.c_int32),
        ("clear_word", C.c_void_p),
    ]


class PredReg(C.Structure):       # lgcn_pred_reg_t
    _fields_ = [
        ("h", C.c_void_p * 8), ("w", C.c_void_p * 8), ("b", C.c_void_p * 8),
        ("ctrs", C.c_void_p), ("wd", C.c_void_p), ("bd", C.c_void_p), ("reg", C.c_void_p), ("hd", C.c_void_p),
        ("n_act", C.c_int64), ("n_mod", C.c_int32), ("np2", C.c_int32),
    ]


class PredRegBwd(C.Structure):    # lgcn_pred_reg_bwd_t
    _fields_ = [
        ("g_reg", C.c_void_p), ("g_hd", C.c_void_p), ("h", C.c_void_p * 8), ("w", C.c_void_p * 8),
        ("hd", C.c_void_p), ("reg", C.c_void_p), ("ctrs", C.c_void_p),
        ("d_h", C.c_void_p * 8), ("d_w", C.c_void_p * 8), ("d_b", C.c_void_p * 8),
        ("d_wd", C.c_void_p), ("d_bd", C.c_void_p), ("part", C.c_void_p),
        ("n_act", C.c_int64), ("n_mod", C.c_int32), ("np2", C.c_int32),
    ]


class AttPairsBwd(C.Structure):   # lgcn_att_pairs_bwd_t
    _fields_ = [
        ("agt_ctrs", C.c_void_p), ("ctx_ctrs", C.c_void_p), ("hi", C.c_void_p), ("wi", C.c_void_p), ("n_pairs", C.c_void_p),
        ("cap", C.c_int64),
        ("wd0", C.c_void_p), ("bd0", C.c_void_p), ("wpd2", C.c_void_p), ("gd", C.c_void_p), ("btd", C.c_void_p),
        ("wpc0e", C.c_void_p), ("U", C.c_void_p), ("V", C.c_void_p), ("gc", C.c_void_p), ("btc", C.c_void_p),
        ("wptd2", C.c_void_p), ("wptc0e", C.c_void_p), ("masks", C.c_void_p), ("dS", C.c_void_p),
        ("dc", C.c_void_p), ("d_wd2", C.c_void_p), ("d_wc0e", C.c_void_p), ("d_wd0", C.c_void_p), ("d_bd0", C.c_void_p),
        ("d_gd", C.c_void_p), ("d_btd", C.c_void_p), ("d_gc", C.c_void_p), ("d_btc", C.c_void_p), ("ws", C.c_void_p),
        ("eps", C.c_float), ("n_chunks", C.c_int32),
    ]


class PoolPairsBwd(C.Structure):  # lgcn_pool_pairs_bwd_t
    _fields_ = [
        ("ctx_pose", C.c_void_p), ("tgt_pose", C.c_void_p), ("ti", C.c_void_p), ("ci", C.c_void_p), ("n_pairs", C.c_void_p),
        ("cap", C.c_int64),
        ("wp", C.c_void_p), ("bp", C.c_void_p), ("wpc0h", C.c_void_p), ("U", C.c_void_p), ("g", C.c_void_p), ("bt", C.c_void_p),
        ("wptc0h", C.c_void_p), ("masks", C.c_void_p), ("dS", C.c_void_p),
        ("dz", C.c_void_p), ("d_w0h", C.c_void_p), ("d_wp", C.c_void_p), ("d_bp", C.c_void_p), ("d_g", C.c_void_p),
        ("d_bt", C.c_void_p), ("ws", C.c_void_p),
        ("eps", C.c_float), ("n_chunks", C.c_int32),
    ]


class LaneConvBwd(C.Structure):   # lgcn_laneconv_bwd_t
    _fields_ = [
        ("d_out", C.c_void_p), ("out", C.c_void_p), ("Z", C.c_void_p), ("Y", C.c_void_p), ("T", C.c_void_p), ("X", C.c_void_p),
        ("gamma1", C.c_void_p), ("gamma2", C.c_void_p), ("wpt2", C.c_void_p), ("wpt1", C.c_void_p),
        ("dT", C.c_void_p), ("g2", C.c_void_p), ("dX", C.c_void_p),
        ("d_w2", C.c_void_p), ("d_w1", C.c_void_p), ("d_g2", C.c_void_p), ("d_b2", C.c_void_p), ("d_g1", C.c_void_p),
        ("d_b1", C.c_void_p), ("ws", C.c_void_p),
        ("n_rows", C.c_int64), ("eps", C.c_float), ("n_chunks", C.c_int32), ("ident1", C.c_int32), ("pad_", C.c_int32),
    ]


class RowBlockBwd(C.Structure):   # lgcn_rowblock_bwd_t
    _fields_ = [
        ("d_out", C.c_void_p), ("out", C.c_void_p), ("pre", C.c_void_p), ("gamma", C.c_void_p),
        ("src", C.c_void_p * 2), ("wpt", C.c_void_p * 2), ("d_src", C.c_void_p * 2), ("d_w", C.c_void_p * 2),
        ("d_res", C.c_void_p), ("d_gamma", C.c_void_p), ("d_beta", C.c_void_p), ("ws", C.c_void_p),
        ("n_rows", C.c_int64), ("ld_w", C.c_int32 * 2), ("eps", C.c_float), ("n_rel", C.c_int32), ("n_chunks", C.c_int32),
        ("pad_", C.c_int32),
    ]


class AggMlp(C.Structure):
    _fields_ = [
        ("n_rows", C.c_int64), ("n_rel", C.c_int32), ("n_rel_csr", C.c_int32),
        ("flags", C.c_int32), ("eps", C.c_float), ("mma", C.c_int32), ("tile_rb", C.c_int32),
        ("rel", Rel * MAX_REL),
        ("rowptr", C.c_void_p), ("col", C.c_void_p),
        ("x4_a", C.c_void_p), ("x4_b", C.c_void_p), ("x4_c", C.c_void_p), ("w4", C.c_void_p),
        ("gn1_g", C.c_void_p), ("gn1_b", C.c_void_p),
        ("wp2", C.c_void_p), ("gn2_g", C.c_void_p), ("gn2_b", C.c_void_p),
        ("res", C.c_void_p), ("out", C.c_void_p), ("out_pre", C.c_void_p),
        ("out_mid", C.c_void_p), ("out_pre2", C.c_void_p),
        ("ch_wq", C.c_void_p), ("ch_gq_g", C.c_void_p), ("ch_gq_b", C.c_void_p), ("ch_wu", C.c_void_p),
        ("ch_u_out", C.c_void_p), ("ch_wv", C.c_void_p), ("ch_v_out", C.c_void_p),
    ]


LC_UNITS = 15


class LaneConv(C.Structure):      # lgcn_laneconv_t
    _fields_ = [
        ("n_rows", C.c_int64), ("x", C.c_void_p), ("wp", C.c_void_p * LC_UNITS),
        ("col", C.c_void_p), ("plan", C.c_void_p),
        ("rows_per_block", C.c_int32), ("cap", C.c_int32), ("n_units", C.c_int32), ("n_groups", C.c_int32),
        ("gstart", C.c_int32 * (LC_UNITS + 1)),
        ("gn1_g", C.c_void_p), ("gn1_b", C.c_void_p), ("wp2", C.c_void_p), ("gn2_g", C.c_void_p), ("gn2_b", C.c_void_p),
        ("eps", C.c_float), ("mma", C.c_int32), ("part", C.c_void_p), ("out", C.c_void_p),
    ]


class OptTensor(C.Structure):     # lgcn_opt_tensor_t
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64)]


class Roi(C.Structure):           # lgcn_roi_t
    _fields_ = [
        ("n_scenes", C.c_int32), ("n_agents", C.c_int32), ("n_nodes", C.c_int32), ("n_lanes", C.c_int32),
        ("n_edges", C.c_int32), ("n_slots", C.c_int32), ("n_suc", C.c_int32), ("n_pre", C.c_int32),
        ("horizon_buffer", C.c_float), ("n_rois", C.c_int32),
        ("n_out_nodes", C.c_int32), ("n_out_edges", C.c_int32), ("n_out_a2m", C.c_int32), ("pad_", C.c_int32),
        ("off_host", C.c_void_p), ("off_dev", C.c_void_p),
        ("ctrs", C.c_void_p), ("feats", C.c_void_p), ("turn", C.c_void_p), ("control", C.c_void_p), ("intersect", C.c_void_p),
        ("lane_idcs", C.c_void_p),
        ("a_ctrs", C.c_void_p), ("a_feats", C.c_void_p), ("a_obs", C.c_void_p),
        ("suc_pairs", C.c_void_p), ("pre_pairs", C.c_void_p), ("edge_u", C.c_void_p), ("edge_v", C.c_void_p),
        ("ws", C.c_void_p),
        ("agent_nodes", C.c_void_p), ("agent_vel", C.c_void_p),
        ("roi_agent", C.c_void_p), ("roi_base", C.c_void_p),
        ("node_mask", C.c_void_p), ("out_feats", C.c_void_p), ("agent_feat", C.c_void_p), ("near", C.c_void_p),
        ("edge_cnt", C.c_void_p),
        ("edge_base", C.c_void_p), ("out_u", C.c_void_p), ("out_v", C.c_void_p), ("a2m_v", C.c_void_p),
    ]


class Store(C.Structure):         # lgcn_store_t
    _fields_ = [
        ("n_scenes", C.c_int64), ("n_nodes", C.c_int64), ("n_actors", C.c_int64), ("n_edges", C.c_int64),
        ("node_ctrs", C.c_void_p), ("node_feats", C.c_void_p), ("turn", C.c_void_p), ("control", C.c_void_p),
        ("intersect", C.c_void_p),
        ("actor_ctrs", C.c_void_p), ("actor_feats", C.c_void_p), ("rot", C.c_void_p), ("orig", C.c_void_p),
        ("gt_preds", C.c_void_p), ("has_preds", C.c_void_p), ("edge_u", C.c_void_p), ("edge_v", C.c_void_p),
    ]


class StoreBatch(C.Structure):    # lgcn_store_batch_t
    _fields_ = [
        ("n_scenes", C.c_int32), ("n_rel", C.c_int32), ("n_nodes", C.c_int64), ("n_actors", C.c_int64), ("n_elem", C.c_int64),
        ("tab_host", C.c_void_p), ("tab_dev", C.c_void_p),
        ("node_ctrs", C.c_void_p), ("node_feats", C.c_void_p), ("turn", C.c_void_p), ("control", C.c_void_p),
        ("intersect", C.c_void_p), ("actor_ctrs", C.c_void_p),
        ("node_off", C.c_void_p), ("actor_off", C.c_void_p),
        ("idx_local", C.c_void_p), ("seg_off", C.c_void_p), ("seg_base", C.c_void_p),
        ("actor_feats", C.c_void_p), ("rot", C.c_void_p), ("orig", C.c_void_p), ("gt_preds", C.c_void_p),
        ("has_preds", C.c_void_p),
    ]


class StorePack(C.Structure):     # lgcn_store_pack_t
    _fields_ = [
        ("n_seg", C.c_int64), ("n_src", C.c_int64), ("n_dst", C.c_int64), ("n_scenes", C.c_int64),
        ("tab_host", C.c_void_p), ("tab_dev", C.c_void_p), ("dst", C.c_void_p), ("frame", C.c_void_p),
        ("rot", C.c_void_p), ("orig", C.c_void_p),
    ]


class RoiStore(C.Structure):      # lgcn_roi_store_t
    _fields_ = [
        ("n_scenes", C.c_int64), ("n_nodes", C.c_int64), ("n_rois", C.c_int64), ("n_edges", C.c_int64), ("n_a2m", C.c_int64),
        ("feats", C.c_void_p), ("node_mask", C.c_void_p), ("agent_feat", C.c_void_p),
        ("edge_u", C.c_void_p), ("edge_v", C.c_void_p), ("a2m_u", C.c_void_p), ("a2m_v", C.c_void_p),
        ("ctrs", C.c_void_p), ("actor_feats", C.c_void_p), ("obs", C.c_void_p), ("gt_preds", C.c_void_p),
        ("has_preds", C.c_void_p),
    ]


class RoiStoreBatch(C.Structure):     # lgcn_roi_store_batch_t
    _fields_ = [
        ("n_scenes", C.c_int64), ("n_nodes", C.c_int64), ("n_rois", C.c_int64), ("n_elem", C.c_int64),
        ("tab_host", C.c_void_p), ("tab_dev", C.c_void_p),
        ("feats", C.c_void_p), ("node_mask", C.c_void_p), ("agent_feat", C.c_void_p), ("idx", C.c_void_p),
        ("ctrs", C.c_void_p), ("actor_feats", C.c_void_p), ("obs", C.c_void_p), ("gt_preds", C.c_void_p),
        ("has_preds", C.c_void_p),
    ]


class SceneTracks(C.Structure):    # lgcn_scene_tracks_t
    _fields_ = [
        ("n_scenes", C.c_int32), ("n_tracks", C.c_int32), ("n_rows", C.c_int32), ("pad_", C.c_int32),
        ("pred_range", C.c_float * 4),
        ("off_host", C.c_void_p), ("off_dev", C.c_void_p), ("xy", C.c_void_p), ("step", C.c_void_p), ("frame", C.c_void_p),
        ("ws", C.c_void_p), ("head", C.c_void_p),
        ("feats", C.c_void_p), ("obs", C.c_void_p), ("ctrs", C.c_void_p), ("gt", C.c_void_p), ("has", C.c_void_p),
    ]


class LaneTableC(C.Structure):     # lgcn_lane_table_t
    _fields_ = [
        ("n_lanes", C.c_int32), ("n_pts", C.c_int32), ("n_pred", C.c_int32), ("n_succ", C.c_int32),
        ("topo_host", C.c_void_p), ("topo_dev", C.c_void_p), ("pts", C.c_void_p),
    ]


class SceneLanes(C.Structure):     # lgcn_scene_lanes_t
    _fields_ = [
        ("n_scenes", C.c_int32), ("n_tables", C.c_int32), ("n_cand", C.c_int32), ("n_rank", C.c_int32),
        ("explicit_ids", C.c_int32), ("pad_", C.c_int32),
        ("pred_range", C.c_double * 4),
        ("tabs_host", C.c_void_p), ("tabs_dev", C.c_void_p), ("off_host", C.c_void_p), ("off_dev", C.c_void_p),
        ("frame", C.c_void_p), ("ws", C.c_void_p), ("head", C.c_void_p),
        ("n_nodes", C.c_int64), ("cap_pre", C.c_int64), ("cap_suc", C.c_int64), ("cap_pre_pairs", C.c_int64),
        ("cap_suc_pairs", C.c_int64), ("cap_left_pairs", C.c_int64), ("cap_right_pairs", C.c_int64),
        ("head2", C.c_void_p),
        ("ctrs", C.c_void_p), ("feats", C.c_void_p), ("turn", C.c_void_p), ("control", C.c_void_p), ("intersect", C.c_void_p),
        ("lane_idcs", C.c_void_p), ("pre_u", C.c_void_p), ("pre_v", C.c_void_p), ("suc_u", C.c_void_p), ("suc_v", C.c_void_p),
        ("pre_pairs", C.c_void_p), ("suc_pairs", C.c_void_p), ("left_pairs", C.c_void_p), ("right_pairs", C.c_void_p),
    ]


class DilateBatch(C.Structure):    # lgcn_dilate_batch_t
    _fields_ = [
        ("n_scenes", C.c_int32), ("pad_", C.c_int32), ("n_nodes", C.c_int64), ("n_pre", C.c_int64), ("n_suc", C.c_int64),
        ("off_host", C.c_void_p), ("off_dev", C.c_void_p),
        ("pre_u", C.c_void_p), ("pre_v", C.c_void_p), ("suc_u", C.c_void_p), ("suc_v", C.c_void_p),
        ("ws", C.c_void_p), ("rowptr", C.c_void_p), ("col", C.c_void_p), ("out_rowptr", C.c_void_p), ("bounds", C.c_void_p),
        ("nnz", C.c_int64), ("out_col", C.c_void_p), ("out_u", C.c_void_p), ("out_v", C.c_void_p),
    ]


class CrossBatch(C.Structure):     # lgcn_cross_batch_t
    _fields_ = [
        ("n_scenes", C.c_int32), ("cross_dist", C.c_float),
        ("n_nodes", C.c_int64), ("n_lanes", C.c_int64), ("n_pre", C.c_int64), ("n_suc", C.c_int64), ("n_left", C.c_int64),
        ("n_right", C.c_int64),
        ("off_host", C.c_void_p), ("off_dev", C.c_void_p), ("ctrs", C.c_void_p), ("feats", C.c_void_p),
        ("lane_idcs", C.c_void_p), ("pre_pairs", C.c_void_p), ("suc_pairs", C.c_void_p), ("left_pairs", C.c_void_p),
        ("right_pairs", C.c_void_p),
        ("mat", C.c_void_p), ("ws", C.c_void_p), ("counts", C.c_void_p), ("out_u", C.c_void_p), ("out_v", C.c_void_p),
    ]


class DaCity(C.Structure):         # lgcn_da_city_t
    _fields_ = [("off", C.c_int64), ("h", C.c_int64), ("w", C.c_int64), ("m", C.c_double * 6)]


class Drivable(C.Structure):       # lgcn_drivable_t
    _fields_ = [("raster", C.c_void_p), ("raster_bytes", C.c_int64), ("city", C.c_void_p), ("city_host", C.c_void_p),
                ("n_cities", C.c_int32), ("scene_city", C.c_void_p)]


OPT_ADAM, OPT_ADAMW, OPT_SGD = 0, 1, 2
OPT_KINDS = {"adam": OPT_ADAM, "adamw": OPT_ADAMW, "sgd": OPT_SGD}

_P, _I, _L, _F, _D = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double

# name -> (restype, argtypes); every symbol include/lgcn.h declares
SIGNATURES = {
    "lgcn_version": (C.c_int, []),
    "lgcn_strerror": (C.c_char_p, [_I]),
    "lgcn_graph_gather": (C.c_int, [_P, _L, _P, _P, _I, _P, _P, _P]),
    "lgcn_csr_rowptr_elems": (C.c_int64, [_L, _I]),
    "lgcn_csr_ws_elems": (C.c_int64, [_L, _I]),
    "lgcn_csr_build": (C.c_int, [_P, _P, _P, _I, _L, _P, _P, _P, _P]),
    "lgcn_pairs_ws_elems": (C.c_int64, [_L, _I]),
    "lgcn_pairs_build": (C.c_int, [_P, _P, _P, _P, _I, _L, _L, _F, _I, _P, _P, _L, _P, _P, _P, _P]),
    "lgcn_pairs_build_multi": (C.c_int, [_P, _I, _P]),
    "lgcn_widen_i32": (C.c_int, [_P, _P, _L, _P, _P]),
    "lgcn_packed_bytes": (C.c_int64, [_I, _I]),
    "lgcn_pack_weight": (C.c_int, [_P, _I, _I, _I, _I, _P, _P]),
    "lgcn_pack_weight_t": (C.c_int, [_P, _I, _I, _P, _P]),
    "lgcn_pack_weight_batch": (C.c_int, [_P, _I, _I, _P]),
    "lgcn_agg_mlp": (C.c_int, [C.POINTER(AggMlp), _P]),
    "lgcn_lc_config": (C.c_int, [_I, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lgcn_lc_plan_elems": (C.c_int64, [_L, _I, _I]),
    "lgcn_lc_part_elems": (C.c_int64, [_L, _I, _I]),
    "lgcn_lc_plan_build": (C.c_int, [_P, _P, _L, _I, _I, _I, _I, C.POINTER(C.c_int32), _P, _P]),
    "lgcn_laneconv_fwd": (C.c_int, [C.POINTER(LaneConv), _P]),
    "lgcn_agg_mlp_pair": (C.c_int, [C.POINTER(AggMlp), C.POINTER(AggMlp), _P]),
    "lgcn_agg_mlp_multi": (C.c_int, [C.POINTER(C.POINTER(AggMlp)), _I, _P]),
    "lgcn_ctx_heads": (C.c_int, [_P, _L, C.POINTER(_P), _I, _I, C.POINTER(_P), _P]),
    "lgcn_node_tail": (C.c_int, [C.POINTER(AggMlp), _P]),
    "lgcn_node_head": (C.c_int, [C.POINTER(C.POINTER(AggMlp)), _I, _P]),
    "lgcn_gn_bwd": (C.c_int, [_P, _P, _P, _P, _L, _F, _P, _P, _P, _P, _P, _P]),
    "lgcn_gn_fwd": (C.c_int, [_P, _P, _P, _P, _L, _F, _I, _P, _P]),
    "lgcn_gn_cl": (C.c_int, [_P, _L, _I, _I, _P, _P, _F, _P, _I, _I, _I, _P, _P]),
    "lgcn_gn_cl_bwd": (C.c_int, [_P, _P, _P, _P, _L, _I, _I, _F, _P, _P, _P, _P]),
    "lgcn_wgrad": (C.c_int, [C.POINTER(AggMlp), _P, _P, _P, _I, _P]),
    "lgcn_gather_rows": (C.c_int, [_P, _P, _P, _L, _P, _P]),
    "lgcn_gather_sum": (C.c_int, [_P, _P, _P, _L, _P, _P]),
    "lgcn_pair_add": (C.c_int, [_P, _P, _P, _P, _P, _P, _L, _P, _P]),
    "lgcn_check_finite": (C.c_int, [_P, _L, _P, _L, _P, _I, _P]),
    "lgcn_check_finite_rows": (C.c_int, [_P, _L, _L, _P, _P, _L, _L, _P, _P, _I, _P]),
    "lgcn_mapnet_input": (C.c_int, [_P, _P, _L] + [_P] * 10 + [_F, _I, _P, _P]),
    "lgcn_att_pairs": (C.c_int, [_P, _P, _P, _P, _P, _L] + [_P] * 10 + [_F, _I, _P, _P]),
    "lgcn_att_pairs_train": (C.c_int, [_P, _P, _P, _P, _P, _L] + [_P] * 10 + [_F, _P, _P, _P]),
    "lgcn_pool_pairs": (C.c_int, [_P, _P, _P, _P, _P, _L] + [_P] * 6 + [_F, _P, _P]),
    "lgcn_pool_pairs_train": (C.c_int, [_P, _P, _P, _P, _P, _L] + [_P] * 6 + [_F, _P, _P, _P]),
    "lgcn_pool_pairs_bwd_ws_elems": (C.c_int64, [_L, _I]),
    "lgcn_pool_pairs_bwd": (C.c_int, [C.POINTER(PoolPairsBwd), _P]),
    "lgcn_att_pairs_bwd_ws_elems": (C.c_int64, [_L, _I]),
    "lgcn_att_pairs_bwd": (C.c_int, [C.POINTER(AttPairsBwd), _P]),
    "lgcn_laneconv_bwd_ws_elems": (C.c_int64, [_L, _I, _I]),
    "lgcn_laneconv_bwd": (C.c_int, [C.POINTER(LaneConvBwd), _P]),
    "lgcn_rowblock_bwd_ws_elems": (C.c_int64, [_L, _I, _I]),
    "lgcn_rowblock_bwd": (C.c_int, [C.POINTER(RowBlockBwd), _P]),
    "lgcn_conv_packed_bytes": (C.c_int64, [_I, _I, _I]),
    "lgcn_conv_pack_weight": (C.c_int, [_P, _I, _I, _I, _P, _P]),
    "lgcn_conv1d_gn": (C.c_int, [_P, _L, _I, _I, _P, _I, _I, _I, _P, _P, _F, _P, _I, _I, _P, _P]),
    "lgcn_conv1d_gn_train": (C.c_int, [_P, _L, _I, _I, _P, _I, _I, _I, _P, _P, _F, _P, _I, _I, _P, _P, _P]),
    "lgcn_conv_packed_t_bytes": (C.c_int64, [_I, _I, _I]),
    "lgcn_conv_pack_weight_t": (C.c_int, [_P, _I, _I, _I, _P, _P]),
    "lgcn_conv1d_gn_bwd_ws_bytes": (C.c_int64, [_L, _I, _I, _I, _I, _I]),
    "lgcn_conv1d_gn_bwd": (C.c_int, [_P, _P, _P, _P, _L, _I, _I, _P, _I, _I, _I, _P, _F, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "lgcn_res1d_gn": (C.c_int, [_P, _L, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _P, _P]),
    "lgcn_res1d_pair_gn": (C.c_int, [_P, _L, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _P, _P]),
    "lgcn_pred_reg": (C.c_int, [C.POINTER(PredReg), _P]),
    "lgcn_pred_final": (C.c_int, [_P, _P, _P, _P, _P, _P, _L, _I, _I, _P, _P, _P]),
    "lgcn_pred_final_train": (C.c_int, [_P, _P, _P, _P, _L, _I, _I, _P, _P, _P, _P]),
    "lgcn_pred_final_bwd_ws_elems": (C.c_int64, [_L]),
    "lgcn_pred_final_bwd": (C.c_int, [_P, _P, _P, _P, _P, _L, _I, _I, _P, _P, _P, _P, _P, _P]),
    "lgcn_pred_reg_bwd_ws_elems": (C.c_int64, [_L, _I, _I]),
    "lgcn_pred_reg_bwd": (C.c_int, [C.POINTER(PredRegBwd), _P]),
    "lgcn_scan_ws_elems": (C.c_int64, [_L]),
    "lgcn_bool_square_bound": (C.c_int, [_P, _P, _L, _P, _P, _P]),
    "lgcn_bool_square": (C.c_int, [_P, _P, _L, _P, _P, _P, _P, _P]),
    "lgcn_bool_square_compact": (C.c_int, [_P, _P, _P, _L, _P, _P, _P]),
    "lgcn_cross_edges": (C.c_int, [_P, _P, _P, _L, _I, _P, _L, _P, _L, _P, _L, _F, _P, _P, _P]),
    "lgcn_index_uv_elems": (C.c_int64, [_L]),
    "lgcn_index_cnt_words": (C.c_int64, [_L, _I]),
    "lgcn_index_build": (C.c_int, [_P, _P]),
    "lgcn_att_pairs_ws": (C.c_int, [_P, _P, _P, _P, _P, _L] + [_P] * 10 + [_F, _I, _I, _P, _P]),
    "lgcn_att_pairs_wi": (C.c_int, [_P, _P, _P, _P, _P, _L] + [_P] * 10 + [_F, _I, _I, _P, _P]),
    "lgcn_pack_weight_kperm": (C.c_int, [_P, _I, _I, _P, _P]),
    "lgcn_pred_loss_fwd": (C.c_int, [_P, _P, _P, _P, _L, _I, _I, _F, _F, _F, _F, _F, _P, _P, _P, _P]),
    "lgcn_pred_loss_bwd": (C.c_int, [_P, _P, _P, _P, _L, _I, _I, _F, _F, _P, _P, _P, _P, _P, _P]),
    "lgcn_conv_packed_f32_bytes": (C.c_int64, [_I, _I, _I]),
    "lgcn_conv_pack_weight_f32": (C.c_int, [_P, _I, _I, _I, _P, _P]),
    "lgcn_conv1d_gn_f32": (C.c_int, [_P, _L, _I, _I, _P, _I, _I, _I, _P, _P, _F, _P, _I, _I, _P, _P, _P]),
    "lgcn_opt_chunk_elems": (C.c_int, []),
    "lgcn_opt_step": (C.c_int, [_P, _I, _P, _I, _I, _D, _D, _D, _D, _D, _D, _I, _D, _D, _I, _F, _F, _P]),
    "lgcn_nms_select": (C.c_int, [_P, _P, _P, _L, _I, _F, _I, _I, _P, _P, _P]),
    "lgcn_goal_decode": (C.c_int, [_P, _P, _P, _L, _P, _P, _L, _P, _P, _P, _P, _P, _I, _I, _F, _P, _P, _P, _P, _P, _P]),
    "lgcn_goal_refine": (C.c_int, [_P, _P, _P, _L, _P, _P]),
    "lgcn_goal_refine_bwd": (C.c_int, [_P, _P, _P, _P, _L, _P, _P, _P, _P]),
    "lgcn_goal_decode_bwd": (C.c_int, [_P, _P, _P, _L, _P, _P, _L, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "lgcn_roi_loss_fwd": (C.c_int, [_P, _P, _P, _P, _P, _L, _I, _I, _F, _P, _P, _P, _P, _P]),
    "lgcn_roi_loss_bwd": (C.c_int, [_P, _P, _P, _P, _P, _L, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P]),
    "lgcn_roi_max_lanes": (C.c_int, []),
    "lgcn_roi_max_levels": (C.c_int, []),
    "lgcn_roi_lane_length_host": (C.c_float, [_P, _P, _I]),
    "lgcn_roi_ws_elems": (C.c_int64, [_L, _L, _L, _L, _L]),
    "lgcn_roi_search": (C.c_int, [C.POINTER(Roi), _P]),
    "lgcn_roi_nodes": (C.c_int, [C.POINTER(Roi), _P]),
    "lgcn_roi_edge_count": (C.c_int, [C.POINTER(Roi), _P]),
    "lgcn_roi_edge_fill": (C.c_int, [C.POINTER(Roi), _P]),
    "lgcn_roi_edge_fill_graph": (C.c_int, [C.POINTER(Roi), _P, _P, _P]),
    "lgcn_store_table_elems": (C.c_int64, [_L, _L]),
    "lgcn_store_gather": (C.c_int, [C.POINTER(Store), C.POINTER(StoreBatch), _P]),
    "lgcn_store_gather_aug": (C.c_int, [C.POINTER(Store), C.POINTER(StoreBatch), _P, _P, _P]),
    "lgcn_store_pad_check": (C.c_int, [C.POINTER(Store), C.POINTER(StoreBatch), _P]),
    "lgcn_store_gather_pad": (C.c_int, [C.POINTER(Store), C.POINTER(StoreBatch), _P]),
    "lgcn_store_pack_table_elems": (C.c_int64, [_L, _L]),
    "lgcn_store_pack": (C.c_int, [C.POINTER(StorePack), _P]),
    "lgcn_roi_store_table_elems": (C.c_int64, [_L]),
    "lgcn_roi_store_gather": (C.c_int, [C.POINTER(RoiStore), C.POINTER(RoiStoreBatch), _P]),
    "lgcn_scene_tracks_ws_elems": (C.c_int64, [_L]),
    "lgcn_scene_tracks": (C.c_int, [C.POINTER(SceneTracks), _P]),
    "lgcn_scene_topo_elems": (C.c_int64, [_L, _L, _L]),
    "lgcn_scene_lanes_ws_elems": (C.c_int64, [_L, _L]),
    "lgcn_scene_lanes_rank": (C.c_int, [C.POINTER(SceneLanes), _P]),
    "lgcn_scene_lanes_fill": (C.c_int, [C.POINTER(SceneLanes), _P]),
    "lgcn_dilate_batch_ws_elems": (C.c_int64, [_L, _L]),
    "lgcn_dilate_batch_csr": (C.c_int, [C.POINTER(DilateBatch), _P]),
    "lgcn_dilate_batch_count": (C.c_int, [C.POINTER(DilateBatch), _P]),
    "lgcn_dilate_batch_fill": (C.c_int, [C.POINTER(DilateBatch), _P]),
    "lgcn_cross_edges_batch_ws_elems": (C.c_int64, [_L]),
    "lgcn_cross_edges_batch": (C.c_int, [C.POINTER(CrossBatch), _P]),
    "lgcn_eval_scenes": (C.c_int, [_P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _L, _P, _P, _P, _P, _P]),
    "lgcn_eval_reduce": (C.c_int, [_P, _L, _D, _P, _P, _P, _P]),
    "lgcn_eval_actors": (C.c_int, [_P, _P, _P, _P, _P, _P, _L, _L, _I, _I, _I, _L, _P, _P, _P, _P, _P]),
    "lgcn_eval_reduce_sel": (C.c_int, [_P, _L, _D, _I, _I, _P, _P, _P, _P]),
    "lgcn_eval_scenes_da": (C.c_int, [_P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _L, _P, _P, _P, _P, C.POINTER(Drivable), _P]),
    "lgcn_eval_actors_da": (C.c_int, [_P, _P, _P, _P, _P, _P, _L, _L, _I, _I, _I, _L, _P, _P, _P, _P, C.POINTER(Drivable), _P]),
    "lgcn_eval_dac_reduce": (C.c_int, [_P, _L, _I, _I, _P, _P]),
}

_lib = None


def load():
    """Load liblgcn.so once; raise LgcnError with build instructions if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LgcnError(
            "liblgcn.so not found at %s -- the HIP extension is required (no CPU fallback). "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C lanegcn-1_amd/csrc`." % LIB_PATH
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().lgcn_strerror(int(rc)).decode()
        raise LgcnError("%s failed: %s (code %d)" % (what, msg, rc))
