/*
 * lgcn.h -- C ABI of the MI355X (gfx950) LaneGCN graph-convolution hot path.
 *
 * This is the drop-in boundary for the path SURVEY.md section 8 scopes:
 * graph_gather -> MapNet (4 x LaneConv) -> A2M -> M2M -> M2A -> A2A of the
 * reference's lanegcn.py.  The reference has no FFI of its own (it is 100 %
 * Python on ATen); each entry point below names the reference lines whose
 * arithmetic it replaces.  The host side (lanegcn-1_amd/, Python) mirrors the
 * reference's nn.Module interface and reaches these symbols through ctypes.
 *
 * Conventions (all entry points):
 *   - extern "C", returns int: 0 = OK, <0 = LGCN_E* (bad argument, nothing
 *     launched), >0 = hipError_t of the failed launch.
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *     the caller owns all memory including workspaces; nothing is allocated,
 *     no global state, no implicit synchronisation, re-entrant.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - feature tensors are row-major fp32 with C = 128 channels (LGCN_C);
 *     indices are int32 inside the library; int64 is accepted/produced at the
 *     edges where the reference's tensors are int64 (utils.py:88-96 to_long).
 *   - kernels are atomic-free on floating point data: results are bitwise
 *     repeatable run to run.
 */
#ifndef LGCN_H
#define LGCN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LGCN_VERSION 100       /* 0.1.0 */
#define LGCN_C 128             /* n_map = n_actor = 128 (lanegcn.py:78-79) */
#define LGCN_TM 16             /* rows of one CSR sub-tile; kernel tiles are 1..4 sub-tiles */
#define LGCN_MAX_REL 16        /* ctr + 14 lane relations (+1 spare) */

enum {
    LGCN_OK = 0,
    LGCN_EINVAL = -1,          /* null pointer / negative size / bad flag */
    LGCN_ESHAPE = -2,          /* size not supported by the kernels */
    LGCN_EALIGN = -3           /* pointer not 16-byte aligned */
};

int lgcn_version(void);
const char *lgcn_strerror(int code);

/* ------------------------------------------------------------------ */
/* Integer path (bit-exact against the reference)                      */
/* ------------------------------------------------------------------ */

/*
 * graph_gather index offsetting, lanegcn.py:191-208:
 *   out[e] = in[e] + base[seg(e)],  seg(e) = the segment with
 *   seg_off[seg] <= e < seg_off[seg+1].
 * One call handles every (relation, u|v, scene) segment of a batch at once:
 * `in` is the concatenation of the per-scene local index arrays, `base` the
 * node offset of the scene each segment belongs to (counts[j], :175-182).
 * out64 and/or out32 may be NULL.
 */
int lgcn_graph_gather(const int64_t *in, int64_t n_elem,
                      const int64_t *seg_off, const int64_t *seg_base, int n_seg,
                      int64_t *out64, int32_t *out32, void *stream);

/*
 * Lane-graph plan: COO (u = destination, v = source) of n_rel relations
 * -> tile-major CSR by destination.  Replaces the 14 index_add_ scatter
 * patterns of lanegcn.py:333-354 / 450-471 by an atomic-free gather.
 *
 *   key(n, r)   = ((n / 16) * n_rel + r) * 16 + n % 16
 *   rowptr      : [n_sub * n_rel * 16 + 1] int32, n_sub = ceil(n_nodes/16)
 *   col         : [sum_r n_edges[r]] int32, sources of row key in ascending
 *                 order of v (duplicates kept: index_add_ adds them twice)
 *
 * u/v of relation r are read from u[r], v[r] (host arrays of device
 * pointers to int64 tensors).  ws: int32 workspace of
 * lgcn_csr_ws_elems(n_nodes, n_rel) elements.
 */
int64_t lgcn_csr_rowptr_elems(int64_t n_nodes, int n_rel);
int64_t lgcn_csr_ws_elems(int64_t n_nodes, int n_rel);
int lgcn_csr_build(const int64_t *const *u_host, const int64_t *const *v_host,
                   const int64_t *n_edges_host, int n_rel, int64_t n_nodes,
                   int32_t *rowptr, int32_t *col, int32_t *ws, void *stream);

/*
 * Att pair search, lanegcn.py:672-689.  For every scene i and every
 * (t, s) in agt_i x ctx_i:  sqrt(fl(dx*dx) + fl(dy*dy)) <= dist_th  in fp32
 * without FMA contraction, pairs emitted in row-major (t, s) order, scenes
 * concatenated.  legacy_offsets != 0 reproduces the reference quirk that a
 * scene with zero pairs does not advance hi_count / wi_count (:681-687).
 *
 *   agt_ctrs [T,2], ctx_ctrs [S,2] fp32: concatenated per-scene centres
 *   agt_off [B+1], ctx_off [B+1] int32: scene offsets into them
 *   hi, wi   : [cap] int32 outputs (cap >= sum_i t_i * s_i is always enough)
 *   n_pairs  : [1] int32 output (device): P
 *   rowptr   : [T+1] int32 output: rowptr[h] = first pair with hi >= h, i.e.
 *              the segments index_add_(0, hi, .) (:703) reduces over
 *   ws       : int32 workspace, lgcn_pairs_ws_elems(T, B) elements
 * If P would exceed cap the pairs beyond cap are dropped, *n_pairs = -P, and rowptr describes the pairs that were kept
 * (every entry <= cap): consumers stay inside [cap, .] buffers; the caller sees the sign, grows cap and runs again.
 */
int64_t lgcn_pairs_ws_elems(int64_t n_agt, int n_scenes);
int lgcn_pairs_build(const float *agt_ctrs, const int32_t *agt_off,
                     const float *ctx_ctrs, const int32_t *ctx_off,
                     int n_scenes, int64_t n_agt, int64_t n_ctx,
                     float dist_th, int legacy_offsets,
                     int32_t *hi, int32_t *wi, int64_t cap,
                     int32_t *n_pairs, int32_t *rowptr, int32_t *ws,
                     void *stream);

/* Several pair searches in the SAME three launches (the forward needs three: A2M, M2A, A2A; each saves the
 * launch boundaries of the others).  `jobs` is a HOST array of n_jobs <= 4 entries; fields as in lgcn_pairs_build. */
typedef struct {
    const float *agt_ctrs; const int32_t *agt_off;
    const float *ctx_ctrs; const int32_t *ctx_off;
    int32_t n_scenes; int32_t legacy_offsets;
    int64_t n_agt, n_ctx;
    float dist_th; int32_t pad_;
    int32_t *hi, *wi; int64_t cap;
    int32_t *n_pairs, *rowptr, *ws;
} lgcn_pairs_job_t;
int lgcn_pairs_build_multi(const lgcn_pairs_job_t *jobs, int n_jobs, void *stream);

/*
 * The whole integer stage of a forward in FOUR launches (count | scan | fill | sort) instead of the twelve of
 * lgcn_graph_gather + lgcn_csr_build + lgcn_pairs_build_multi; bit-identical outputs.
 *   idx_local [n_elem], seg_off / seg_base [n_seg]: as lgcn_graph_gather (reference lanegcn.py:191-208); relation r's
 *     destination indices are elements u_off[r] .. u_off[r] + n_edges[r] of the gathered array, its sources start at
 *     v_off[r] (the global indices are formed on the fly and not written out).
 *   rowptr [lgcn_csr_rowptr_elems], col [sum n_edges]: the plan of lgcn_csr_build.
 *   cnt   : lgcn_index_cnt_words(n_nodes, n_rel) 64-bit words, 8-byte aligned.  MUST BE ALL ZERO on entry; the
 *           launches leave it all zero again, so a buffer serves call after call without a zeroing launch (one
 *           buffer per forward that can be in flight).
 *   uv    : int32 workspace, lgcn_index_uv_elems(sum n_edges) elements.
 *   jobs  : up to four pair searches (HOST array, as lgcn_pairs_build_multi); n_jobs may be 0.
 * Limit of this entry point (LGCN_ESHAPE beyond it; use the separate calls there): lgcn_csr_rowptr_elems <= 2^22.
 */
typedef struct {
    const int64_t *idx_local; int64_t n_elem;
    const int64_t *seg_off, *seg_base; int32_t n_seg, n_rel;
    int64_t u_off[LGCN_MAX_REL], v_off[LGCN_MAX_REL], n_edges[LGCN_MAX_REL];
    int64_t n_nodes;
    int32_t *rowptr, *col;
    void *cnt;
    int32_t *uv;
    const lgcn_pairs_job_t *jobs; int32_t n_jobs, pad_;
    int32_t *clear_word;     /* optional (may be NULL): a 32-bit word the first launch sets to 0 -- the forward's
                                range-guard flag (lgcn_check_finite) rides along instead of costing a fill launch */
} lgcn_index_t;
int64_t lgcn_index_uv_elems(int64_t n_edges);
int64_t lgcn_index_cnt_words(int64_t n_nodes, int n_rel);
int lgcn_index_build(const lgcn_index_t *p_host, void *stream);

/* ------------------------------------------------------------------ */
/* ActorNet's convolution block           */
/* ------------------------------------------------------------------ */

/*
 * layers.Conv1d / one half of layers.Res1d of the reference (layers.py:40-62, 142-190; ActorNet lanegcn.py:212-263)
 * in one launch, on channels-last tensors:
 *   out[a, l, :] = act( GN( sum_t W[:, :, t] x[a, l * stride + t - pad, :] ) + residual ),  pad = (ks - 1) / 2
 * x [A, lin, cin] fp32, out [A, lout, cout], lout = (lin + 2 pad - ks) / stride + 1; GN = GroupNorm(1, cout): statistics
 * over the lout x cout values of an actor (biased variance, eps), gamma / beta [cout].
 * Supported: ks in {1, 3}, stride in {1, 2}, cin <= 128, cout in {32, 64, 128}, lout in {5, 10, 20} (ActorNet's three pyramid levels);
 * anything else: LGCN_ESHAPE.  wp: lgcn_conv_pack_weight image of W [cout, cin, ks] (lgcn_conv_packed_bytes bytes).
 * res_mode 0: no residual; 1: res [A, lout, cout]; 2: res [A, lout / 2, cout], upsampled x2 as
 * F.interpolate(mode = "linear", align_corners = False) (the FPN's top-down step, lanegcn.py:256-260).  relu != 0: ReLU last.
 * Arithmetic: fp16 operand planes (2 planes, 3 products, fp32 accumulate: fp32-grade inside LGCN_MMA_F16X2's operand window, see below).
 */
int64_t lgcn_conv_packed_bytes(int cin, int cout, int ks);
int lgcn_conv_pack_weight(const float *w, int cin, int cout, int ks, void *out, void *stream);
int lgcn_conv1d_gn(const float *x, int64_t n_act, int lin, int cin, const void *wp, int cout, int ks, int stride,
                   const float *gamma, const float *beta, float eps, const float *res, int res_mode, int relu,
                   float *out, void *stream);

/*
 * Training forward: lgcn_conv1d_gn that also stores the pre-norm convolution output y [A, lout, cout] (y = sum_t W_t x
 * shifted, before the GroupNorm).  Same kernel, one extra store: `out` is bit-identical to lgcn_conv1d_gn's.  Same shape set,
 * pointer and alignment checks; y must be non-null and 16-byte aligned.
 */
int lgcn_conv1d_gn_train(const float *x, int64_t n_act, int lin, int cin, const void *wp, int cout, int ks, int stride,
                         const float *gamma, const float *beta, float eps, const float *res, int res_mode, int relu,
                         float *out, float *y, void *stream);

/*
 * Backward of lgcn_conv1d_gn_train (reference layers.py:40-62, 142-190; lanegcn.py:212-263).  Given g = dL/dout [A, lout, cout]
 * and the forward's x, y, out:
 *   gm     = g masked by out > 0 (relu != 0; out may be NULL otherwise)
 *   dres   = gm (res_mode 1, [A, lout, cout]), or for res_mode 2 the adjoint of the x2 upsampling of lgcn_gn_cl:
 *            dres[h] = sum_l gm[l] (w0(l) [i0(l) == h] + w1(l) [i1(l) == h])  ([A, lout / 2, cout], edges clamped)
 *   dy     = rstd (gm gamma - mean_a(gm gamma) - yhat mean_a(gm gamma yhat)),  yhat = (y - mean_a) rstd  (per actor, two-pass
 *            statistics of y as the forward computed them)
 *   dx     [A, lin, cin]:  dx[a, li, ci] = sum_{t, l: l stride + t - pad = li} sum_co dy[a, l, co] W[co, ci, t]
 *   dW     [cout, cin, ks] (the parameter's layout):  dW[co, ci, t] = sum_{a, l} dy[a, l, co] x[a, l stride + t - pad, ci]
 *   dgamma = sum_{a, l} gm yhat,  dbeta = sum_{a, l} gm     ([cout])
 * dx, dres, dw, dgamma, dbeta may each be NULL (not computed); x is needed only for dw.  wt: lgcn_conv_pack_weight_t image of W
 * (lgcn_conv_packed_t_bytes bytes: fp32 wt[t][ci][co], ci padded to a multiple of 16 with zeros).  ws: workspace of
 * lgcn_conv1d_gn_bwd_ws_bytes(n_act, lin, cin, cout, ks, stride) bytes (dy, per-workgroup dgamma / dbeta partials, chunked dW
 * partials), 16-byte aligned.  Shapes, res_mode and pointer checks as lgcn_conv1d_gn.  Three launches: the data backward
 * (workgroups of whole actors as in the forward), the weight gradient in chunks, the fixed-order reduction of all
 * partials.  Arithmetic: exact fp32 (v_mfma_f32_16x16x4_f32), no floating-point atomics: bitwise repeatable.
 */
int64_t lgcn_conv_packed_t_bytes(int cin, int cout, int ks);
int lgcn_conv_pack_weight_t(const float *w, int cin, int cout, int ks, void *out, void *stream);
int64_t lgcn_conv1d_gn_bwd_ws_bytes(int64_t n_act, int lin, int cin, int cout, int ks, int stride);
int lgcn_conv1d_gn_bwd(const float *g, const float *x, const float *y, const float *out, int64_t n_act, int lin, int cin,
                       const void *wt, int cout, int ks, int stride, const float *gamma, float eps, int res_mode, int relu,
                       float *dx, float *dw, float *dgamma, float *dbeta, float *dres, void *ws, void *stream);

/*
 * A whole layers.Res1d block (reference layers.py:142-190) in one launch, same layouts and shape limits as
 * lgcn_conv1d_gn:  out = relu( GN2(conv2( relu(GN1(conv1 x)) )) + r ),  conv1: k = 3, stride 1 / 2, cin -> c; conv2: k = 3,
 * stride 1, c -> c; r = x (wdp == NULL: needs cin == c, stride 1) or GN_d(conv_d x) with conv_d: k = 1, same stride
 * (wdp, gd, bd given).  c in {32, 64, 128}; w1p / w2p / wdp: lgcn_conv_pack_weight images.  The intermediate stays in LDS
 * (one region of <= 46 KB serves as input planes, tiles and intermediate planes in turn).
 */
int lgcn_res1d_gn(const float *x, int64_t n_act, int lin, int cin, int c, int stride, const void *w1p, const float *g1,
                  const float *b1, const void *w2p, const float *g2, const float *b2, const void *wdp, const float *gd,
                  const float *bd, float eps, float *out, void *stream);
/* Two Res1d blocks in one launch: the block above followed by a second one with the identity shortcut (c -> c, stride 1;
 * w1q .. b2q: its conv1 / GN1 / conv2 / GN2) -- a group of ActorNet (lanegcn.py:228-241).  Only the second block's output
 * is written. */
int lgcn_res1d_pair_gn(const float *x, int64_t n_act, int lin, int cin, int c, int stride, const void *w1p, const float *g1,
                       const float *b1, const void *w2p, const float *g2, const float *b2, const void *wdp, const float *gd,
                       const float *bd, const void *w1q, const float *g1q, const float *b1q, const void *w2q, const float *g2q,
                       const float *b2q, float eps, float *out, void *stream);

/* ------------------------------------------------------------------ */
/* PredNet's tail                         */
/* ------------------------------------------------------------------ */

/*
 * The stock-op remainder of PredNet.forward (reference lanegcn.py:575-631), AttDest's first layer (lanegcn.py:725-729)
 * and Net.forward's world-frame transform (lanegcn.py:147-150), inference.  The LinearRes / Linear + GroupNorm stages
 * between the two calls are lgcn_agg_mlp row blocks.
 *
 * lgcn_pred_reg: for every mode m < n_mod (<= 8) and actor a
 *   reg[a, m, :]  = w[m] h[m][a] + b[m] + (ctr[a].x, ctr[a].y, ctr[a].x, ...)     h[m] [A, 128], w[m] [np2, 128], b[m] [np2]
 *   hd[a n_mod + m, :] = relu(wd (ctr[a] - reg[a, m, np2 - 2 : np2]) + bd)         wd [128, 2], bd [128]: AttDest.dist[0]
 * np2 = 2 * num_preds, even, <= 64.  reg [A, n_mod, np2], hd [A n_mod, 128], ctrs [A, 2], all fp32.
 */
typedef struct lgcn_pred_reg {
    const float *h[8];
    const float *w[8];
    const float *b[8];
    const float *ctrs;
    const float *wd, *bd;
    float *reg, *hd;
    int64_t n_act;
    int32_t n_mod, np2;
} lgcn_pred_reg_t;
int lgcn_pred_reg(const lgcn_pred_reg_t *q, void *stream);

/*
 * lgcn_pred_final: scores cls[a, m] = wc . f[a n_mod + m, :] + bc (the nn.Linear(128, 1) of PredNet.cls), sorted
 * descending per actor (equal scores keep mode order), reg's modes gathered in that order (lanegcn.py:614-625) and,
 * when rot / orig are given ([A, 2, 2], [A, 2]: each actor's scene rotation and origin), taken to world coordinates:
 * out[a, j, t, :] = reg[a, order_j, t, :] rot[a] + orig[a].  rot == orig == NULL: no transform.
 * f [A n_mod, 128], reg / out [A, n_mod, n_pred, 2], cls [A, n_mod].
 */
int lgcn_pred_final(const float *f, const float *wc, const float *bc, const float *reg, const float *rot, const float *orig,
                    int64_t n_act, int n_mod, int n_pred, float *cls, float *out, void *stream);

/*
 * Training forward of the final launch (reference lanegcn.py:614-625): lgcn_pred_final without rot / orig that also
 * stores order [A, n_mod] int32, order[a, j] = the mode whose score took rank j (cls[a, j] = s[a, order[a, j]],
 * out[a, j] = reg[a, order[a, j]]).  Same kernel, one extra store: cls / out are bit-identical to lgcn_pred_final's.
 * np2 = 2 * num_preds, even, 2..64 (the shape set of lgcn_pred_reg, which serves the training forward unchanged).
 */
int lgcn_pred_final_train(const float *f, const float *wc, const float *bc, const float *reg, int64_t n_act, int n_mod,
                          int np2, float *cls, float *out, int32_t *order, void *stream);

/*
 * Backward of lgcn_pred_final_train (the sort and gather of lanegcn.py:618-622, the score nn.Linear(128, 1) of :599).
 * Given g_cls [A, n_mod] and g_out [A, n_mod, np2] (either may be NULL: taken as zeros), the forward's order, f and wc:
 *   g_s[a, order[a, j]] = g_cls[a, j],   g_reg[a, order[a, j], :] = g_out[a, j, :]        (g_reg [A, n_mod, np2])
 *   d_f[a n_mod + m, :] = g_s[a, m] wc                                                     (d_f [A n_mod, 128])
 *   d_wc[c] = sum_rows g_s f[row, c],  d_bc = sum g_s                                      ([128], [1])
 * Every element of g_reg and d_f is written (no memset needed); g_reg / d_f may be NULL (not computed).  part: workspace
 * of lgcn_pred_final_bwd_ws_elems(n_act) floats.  Two launches: the per-actor pass with per-workgroup partials of
 * d_wc / d_bc, and their reduction in a fixed order.  Plain fp32, no floating-point atomics: bitwise repeatable.
 * g_out, f, wc, g_reg, d_f 8-byte aligned.
 */
int64_t lgcn_pred_final_bwd_ws_elems(int64_t n_act);
int lgcn_pred_final_bwd(const float *g_cls, const float *g_out, const int32_t *order, const float *f, const float *wc,
                        int64_t n_act, int n_mod, int np2, float *g_reg, float *d_f, float *d_wc, float *d_bc, float *part,
                        void *stream);

/*
 * Backward of lgcn_pred_reg (the heads' nn.Linear(128, 2 T) and the centre add of lanegcn.py:601-612, AttDest.dist[0] of
 * :725-729).  The reference detaches the destination before AttDest (:614), so hd carries gradient to wd / bd only.
 * Given g_reg [A, n_mod, np2], g_hd [A n_mod, 128] (may be NULL: taken as zeros) and the forward's h, w, hd, reg, ctrs:
 *   d_h[m][a, :] = sum_o g_reg[a, m, o] w[m][o, :]
 *   d_w[m][o, :] = sum_a g_reg[a, m, o] h[m][a, :],   d_b[m][o] = sum_a g_reg[a, m, o]
 *   p = g_hd (hd > 0),  d = ctr[a] - reg[a, m, np2 - 2 : np2]:
 *   d_wd[c, :] = sum_rows p[row, c] d[row, :],        d_bd[c] = sum_rows p[row, c]
 * Every output pointer may be NULL: that gradient is not computed (all d_h NULL skips the data gradient, all d_w / d_b
 * NULL the contraction over actors, d_wd and d_bd NULL the AttDest part).  part: workspace of
 * lgcn_pred_reg_bwd_ws_elems(n_act, n_mod, np2) floats, 16-byte aligned, as are h, w and d_h.  Two launches: workgroups
 * of (chunk of actors, mode) that write d_h and one partial record per chunk, and the reduction of the records in chunk
 * order.  Plain fp32 FMA chains, no floating-point atomics: bitwise repeatable.
 */
typedef struct lgcn_pred_reg_bwd {
    const float *g_reg;
    const float *g_hd;
    const float *h[8];
    const float *w[8];
    const float *hd, *reg, *ctrs;
    float *d_h[8];
    float *d_w[8];
    float *d_b[8];
    float *d_wd, *d_bd;
    float *part;
    int64_t n_act;
    int32_t n_mod, np2;
} lgcn_pred_reg_bwd_t;
int64_t lgcn_pred_reg_bwd_ws_elems(int64_t n_act, int n_mod, int np2);
int lgcn_pred_reg_bwd(const lgcn_pred_reg_bwd_t *q, void *stream);

/* ------------------------------------------------------------------ */
/* Graph construction on the device       */
/* ------------------------------------------------------------------ */

/*
 * One boolean squaring of a CSR adjacency: the step of data.dilated_nbrs (reference data.py:520-534: the scale-i
 * relation is A^(2^i), `mat = mat * mat` per scale; u = row, v = column).  Rows may be unsorted and hold duplicates.
 *   1. lgcn_bool_square_bound  : cand_ptr [n+1] = exclusive scan of the rows' candidate counts; read cand_ptr[n] on
 *                                the host and allocate cand [cand_ptr[n]].
 *   2. lgcn_bool_square        : out_rowptr [n+1] = rowptr of A*A (boolean: each entry once, columns ascending); read
 *                                out_rowptr[n] = nnz and allocate out_col [nnz] (and out_row for a COO).
 *   3. lgcn_bool_square_compact: out_col (and out_row, may be NULL) filled.
 * ws: int32 workspace of lgcn_scan_ws_elems(n + 1) elements.  Entries that point outside [0, n) are ignored.
 */
int64_t lgcn_scan_ws_elems(int64_t n);
int lgcn_bool_square_bound(const int32_t *rowptr, const int32_t *col, int64_t n, int32_t *cand_ptr, int32_t *ws,
                           void *stream);
int lgcn_bool_square(const int32_t *rowptr, const int32_t *col, int64_t n, const int32_t *cand_ptr, int32_t *cand,
                     int32_t *out_rowptr, int32_t *ws, void *stream);
int lgcn_bool_square_compact(const int32_t *cand_ptr, const int32_t *cand, const int32_t *out_rowptr, int64_t n,
                             int32_t *out_col, int32_t *out_row, void *stream);

/*
 * Left (or right) node adjacency of one scene: reference preprocess_data.py:287-392 with cross_angle = None, for the
 * side whose lane pairs are passed (left_pairs or right_pairs; call twice).
 *   ctrs, feats [n_nodes,2] (segment midpoints / vectors), lane_idcs [n_nodes] int64 (lane of every node),
 *   side_pairs / pre_pairs / suc_pairs: [k,2] int64 lane pairs; mat: num_lanes^2 bytes of workspace.
 *   partner [n_nodes]: the node v that node u is linked to (edge u -> v of the reference's `left`/`right` dict), or -1:
 *   the nearest centre among the nodes of the lanes (S pre + S suc + S)[lane(u)] allows, if it is closer than
 *   cross_dist and the two headings differ by less than pi / 4.  Distances are formed exactly as ATen does (fp32,
 *   no FMA), ties go to the smaller node index; the heading test uses atan2f (its last bit may differ from ATen's).
 */
int lgcn_cross_edges(const float *ctrs, const float *feats, const int64_t *lane_idcs, int64_t n_nodes, int num_lanes,
                     const int64_t *side_pairs, int64_t n_side, const int64_t *pre_pairs, int64_t n_pre,
                     const int64_t *suc_pairs, int64_t n_suc, float cross_dist, uint8_t *mat, int32_t *partner,
                     void *stream);

/* int32 -> int64 widening of the first *n (device count, clamped to cap)
 * entries; the tail is left untouched.  Used to hand hi/wi back as the
 * reference's LongTensors. */
int lgcn_widen_i32(const int32_t *in, const int32_t *n_dev, int64_t cap,
                   int64_t *out, void *stream);

/* ------------------------------------------------------------------ */
/* Floating point path (fp32 in / fp32 out; tolerance 1e-4 on features) */
/* ------------------------------------------------------------------ */

/*
 * How the 128-d Linear contractions are evaluated on the matrix cores:
 *   LGCN_MMA_F32    v_mfma_f32_32x32x2_f32: bit-exact fp32 fma chain (64 FLOP/clk/SIMD).
 *   LGCN_MMA_BF16X3 both operands split into 3 bf16 terms (x = hi + mid + lo, 24 mantissa
 *                   bits), 6 products hi*hi, hi*mid, mid*hi, hi*lo, lo*hi, mid*mid on
 *                   v_mfma_f32_16x16x32_bf16 with fp32 accumulation: fp32-grade result
 *                   (dropped terms <= 2^-24 relative) at 2.67x the f32 MFMA rate.
 *   LGCN_MMA_BF16   one bf16 product (BASELINE config "bf16"; ~2e-2 relative on features).
 *   LGCN_MMA_F16X2  both operands split into 2 fp16 terms (x = hi + lo, 22 mantissa bits),
 *                   3 products hi*hi, hi*lo, lo*hi on v_mfma_f32_16x16x32_f16, fp32 accumulation:
 *                   fp32-grade (dropped terms <= 2^-22 relative; measured equal to fp32's own
 *                   reordering noise on this path) with 2/3 of the weight bytes and half the
 *                   MFMAs of BF16X3.  Operand window: |x| < 65520 (the first fp32 value that rounds to
 *                   fp16's infinity), and, because the planes' quantum stops shrinking below fp16's normal
 *                   range, within 1e-4 of the output's scale only while max |W| of a weight block >= 2^-9
 *                   (2e-3) and max |x| >= 2^-10 with the other operand O(1) (1e-3 at max |W| = 2^-13, 1e-2 at
 *                   2^-17; subnormal planes are kept).  True behind this network's GroupNorms with weights of
 *                   ordinary size; use BF16X3 or F32 for unbounded inputs or small weight blocks.
 */
enum { LGCN_MMA_F32 = 0, LGCN_MMA_BF16X3 = 1, LGCN_MMA_BF16 = 2, LGCN_MMA_F16X2 = 3 };

/*
 * Weight prepacking.  W is an nn.Linear weight [128, k_real] with row stride
 * ld (floats).
 * LGCN_MMA_F32: the image feeds v_mfma_f32_32x32x2_f32 with one 16-byte load
 * per lane per 8 k's:
 *   out[w][q][lane][j] = W[32*w + (lane & 31)][8*q + 4*(lane >> 5) + j]   (fp32)
 * for w < 4, q < k_pad/8, j < 4 (zero for k >= k_real), k_pad % 8 == 0;
 * out holds 128 * k_pad floats.
 * LGCN_MMA_BF16X3 / LGCN_MMA_F16X2 / LGCN_MMA_BF16: k_real = k_pad = 128; 3 / 2 / 1
 * 16-bit planes of the split for v_mfma_f32_16x16x32_{bf16,f16}:
 *   out[p][w][s][cb][lane][j] = plane_p(W[32*w + 16*cb + (lane & 15)][32*s + 8*(lane >> 4) + j])
 * p < planes, w < 4, s < 4, cb < 2, j < 8; out holds planes * 32 KiB.
 */
int64_t lgcn_packed_bytes(int k_pad, int mma);
int lgcn_pack_weight(const float *W, int ld, int k_real, int k_pad, int mma,
                     void *out, void *stream);
/* Same, for the TRANSPOSE of a square [128,128] weight (W[k][j] read in place of W[j][k]): the
 * backward of y = x W^T is dx = dy W, i.e. a Linear whose weight is W^T. */
int lgcn_pack_weight_t(const float *W, int ld, int mma, void *out, void *stream);

/* Many [128,128] blocks in one launch: what a training loop does after every optimizer step (train.py:190,
 * the weights change in place) instead of ~400 single launches.  `jobs` is a DEVICE array. */
typedef struct {
    const float *W;          /* top-left element of the [128,128] block (row stride ld) */
    void *out;               /* packed image, lgcn_packed_bytes(128, mma) bytes         */
    int32_t ld;
    int32_t transpose;       /* 0: lgcn_pack_weight, 1: lgcn_pack_weight_t             */
} lgcn_pack_job_t;
int lgcn_pack_weight_batch(const lgcn_pack_job_t *jobs, int n_jobs, int mma, void *stream);

/* One relation of an aggregate-GEMM stage (see lgcn_agg_mlp). */
typedef struct {
    const float *src;        /* [*,128] source rows                        */
    const float *wp;         /* packed weight, k_pad = 128                 */
    int32_t mode;            /* LGCN_REL_*                                 */
    int32_t ridx;            /* LGCN_REL_CSR: relation index in the plan   */
} lgcn_rel_t;

enum {
    LGCN_REL_IDENT = 0,      /* A[n] = src[n]                              */
    LGCN_REL_CSR = 1,        /* A[n] = sum_{e in row key(n,ridx)} src[col[e]] */
    LGCN_REL_RANGE = 2,      /* A[n] = sum_{p in [rowptr[n],rowptr[n+1])} src[p] */
    LGCN_REL_RANGE16 = 3     /* as RANGE over a src written by lgcn_att_pairs_ws(seg = 16): of a segment [b, e) only
                                rows b and the multiples of 16 inside (b, e) hold data (sums of 16-aligned pieces);
                                split-precision modes only (F32: LGCN_ESHAPE) */
};

enum {                        /* lgcn_agg_mlp flags                         */
    LGCN_F_GN1 = 1, LGCN_F_RELU1 = 2, LGCN_F_GEMM2 = 4, LGCN_F_GN2 = 8,
    LGCN_F_RES = 16, LGCN_F_RELU2 = 32
};

typedef struct {
    int64_t n_rows;          /* N destination rows                         */
    int32_t n_rel;           /* 1..LGCN_MAX_REL                            */
    int32_t n_rel_csr;       /* relations in the CSR plan (rowptr layout)  */
    int32_t flags;           /* LGCN_F_*                                   */
    float eps;               /* GroupNorm eps (1e-5)                       */
    int32_t mma;             /* LGCN_MMA_* (all wp / wp2 packed for it)    */
    int32_t tile_rb;         /* bf16 modes: 16-row blocks per tile, 1..4; 0 = pick by occupancy */
    lgcn_rel_t rel[LGCN_MAX_REL];
    const int32_t *rowptr;   /* CSR plan rowptr, or [N+1] for RANGE        */
    const int32_t *col;      /* CSR plan col                               */
    const float *x4_a;       /* optional [N,2] extra inputs (A2M meta:     */
    const float *x4_b;       /*   turn[N,2], control[N], intersect[N])     */
    const float *x4_c;
    const float *w4;         /* [128,4] weight columns for them, or NULL   */
    const float *gn1_g, *gn1_b;
    const float *wp2;        /* packed stage-2 weight                      */
    const float *gn2_g, *gn2_b;
    const float *res;        /* [N,128] residual                           */
    float *out;              /* [N,128]                                    */
    float *out_pre;          /* optional [N,128]: stage-1 sums T (pre-GN1)  (saved for backward) */
    float *out_mid;          /* optional [N,128]: Y = act(GN1(T)), the stage-2 operand          */
    float *out_pre2;         /* optional [N,128]: Z = Y W2^T (pre-GN2)                          */
    /* Optional CHAINED outputs, computed from the block's final rows y (= out) before they leave the CU -- what the
     * NEXT Att layer needs from these rows (reference lanegcn.py:696-699, after hoisting the row-wise Linears out of
     * the pair loop: see lgcn_att_pairs):
     *   ch_u_out = ReLU(GN_q(y W_q^T)) W_u^T    that layer's query + its ctx.0[:, 128:256] part (y are its targets)
     *   ch_v_out = y W_v^T                      that layer's ctx.0[:, 256:384] part (y are its context rows: A2A)
     * ch_wu != NULL selects the first (needs ch_wq, ch_gq_g, ch_gq_b, ch_u_out), ch_wv != NULL the second (needs
     * ch_v_out).  Same arithmetic as separate lgcn_agg_mlp launches on `out`; saves their launches. */
    const float *ch_wq, *ch_gq_g, *ch_gq_b, *ch_wu;
    float *ch_u_out;
    const float *ch_wv;
    float *ch_v_out;
} lgcn_agg_mlp_t;

/*
 * Fused "aggregate -> GEMM -> GN -> ReLU -> GEMM -> GN -> +res -> ReLU" row
 * block.  With the 15 relations ctr, pre0, suc0, ..., left, right it is one
 * LaneConv layer (lanegcn.py:331-362 == 448-479):
 *   T = sum_r (sum_{e:u=n} X[v]) W_r^T ; Y = ReLU(GN1(T)) ;
 *   out = ReLU(GN2(Y W2^T) + res)
 * With {IDENT(a, W_agt), RANGE(m, W_c1)} it is the tail of Att.forward
 * (:702-709); with one IDENT relation and subsets of the flags it is
 * layers.Linear (layers.py:65-87), Att.query (:696), A2M.meta (:387-395).
 */
int lgcn_agg_mlp(const lgcn_agg_mlp_t *p_host, void *stream);

/*
 * LaneConv layer, gather-free and weight-stationary (reference lanegcn.py:331-362 == 448-479; the same arithmetic as
 * lgcn_agg_mlp with the 15 relations, cut differently -- see csrc/lgcn_laneconv.hip):
 *   T = sum_u (G_u X) W_u^T ;  Y = ReLU(GN1(T)) ;  out = ReLU(GN2(Y W2^T) + X)
 * UNITS: u = 0 is ctr (the row itself), u = 1 + r is relation r of the lgcn_csr_build plan (pre0, suc0, ..., left,
 * right).  Rows are cut into ROW BLOCKS of rows_per_block rows; a work item is (row block, run of consecutive
 * units): its workgroup keeps every unit's weight slice in registers for the whole row block and reads the MFMA row
 * operands straight from the item's DISTINCT source rows, which it loads once into LDS.  lgcn_lc_plan_build lists
 * those rows once per batch (the lane graph is the same for the 8 LaneConv layers of a forward).
 *
 *   lgcn_lc_config      rows_per_block and the LDS source-row capacity of a shape in a matrix mode (BF16X3 / F16X2 /
 *                       BF16; F32 is not supported here: LGCN_ESHAPE, use lgcn_agg_mlp).  variant 0 "shared": 96-row
 *                       blocks (64 in BF16X3), two workgroups per CU; 1 "tall": 192 (128) rows, the whole CU, half
 *                       the weight traffic per row, for batches with >= 2 such blocks per CU; 2 "short": 48 (32) rows
 *                       within the shared budget: one block per CU finishes a small batch's layer in one launch.
 *   lgcn_lc_plan_build  rowptr / col: the lgcn_csr_build plan of n_rel relations (n_units = n_rel + 1 <= 15).
 *                       gstart_host[0..n_groups]: unit groups, gstart[0] = 0 < ... < gstart[n_groups] = n_units;
 *                       one workgroup per (row block, group).  n_groups = 1: a workgroup runs all units of its row
 *                       block and finishes the layer itself (one launch, no partial sums); n_groups > 1: more
 *                       parallelism for small batches, the groups' fp32 partial sums are added by a second launch.
 *                       cap: source rows an item may hold, rows_per_block <= cap <= the mode's capacity; a group
 *                       whose distinct sources exceed it is split into several items that the same workgroup runs
 *                       one after the other (the results do not depend on cap or on the grouping beyond fp32
 *                       summation order).  plan: lgcn_lc_plan_elems() int32 words, 16-byte aligned.
 *   lgcn_laneconv_fwd   one layer: x [N,128] in, out [N,128]; wp[u] packed W_u (may be NULL for a relation without
 *                       edges); part: workspace of lgcn_lc_part_elems() floats (unused when n_groups = 1).
 *                       rows_per_block, cap, n_groups and gstart must be the ones the plan was built with.
 *                       No atomics: bitwise repeatable.
 */
#define LGCN_LC_UNITS 15
typedef struct {
    int64_t n_rows;
    const float *x;                   /* [N,128] layer input (also the residual) */
    const float *wp[LGCN_LC_UNITS];   /* packed weights per unit                 */
    const int32_t *col;               /* lgcn_csr_build col                      */
    const int32_t *plan;              /* lgcn_lc_plan_build output               */
    int32_t rows_per_block, cap, n_units, n_groups;
    int32_t gstart[LGCN_LC_UNITS + 1];
    const float *gn1_g, *gn1_b;
    const float *wp2;
    const float *gn2_g, *gn2_b;
    float eps;
    int32_t mma;
    float *part;                      /* workspace                               */
    float *out;                       /* [N,128]                                 */
} lgcn_laneconv_t;
int lgcn_lc_config(int mma, int variant, int32_t *rows_per_block, int32_t *cap);
int64_t lgcn_lc_plan_elems(int64_t n_nodes, int rows_per_block, int cap);
int64_t lgcn_lc_part_elems(int64_t n_nodes, int rows_per_block, int n_groups);
int lgcn_lc_plan_build(const int32_t *rowptr, const int32_t *col, int64_t n_nodes, int n_rel,
                       int rows_per_block, int cap, int n_groups, const int32_t *gstart_host,
                       int32_t *plan, void *stream);
int lgcn_laneconv_fwd(const lgcn_laneconv_t *p_host, void *stream);

/* Two independent row blocks (e.g. Att's per-target U and per-context V, lanegcn.py:696-699) in ONE launch when both
 * are split-precision problems without CSR relations; otherwise the same as two lgcn_agg_mlp calls. */
int lgcn_agg_mlp_pair(const lgcn_agg_mlp_t *a_host, const lgcn_agg_mlp_t *b_host, void *stream);

/* Up to LGCN_MAX_MULTI independent row blocks in ONE launch (the head of a fusion block: A2M.meta chained into the
 * first Att's U, and the V rows of both of its Att layers, lanegcn.py:387-406), under the conditions of
 * lgcn_agg_mlp_pair; otherwise the same as n lgcn_agg_mlp calls in order. */
#define LGCN_MAX_MULTI 4
int lgcn_agg_mlp_multi(const lgcn_agg_mlp_t *const *ps_host, int n, void *stream);

/*
 * Context heads of an Att block whose context rows are not its targets (M2A: the lane nodes; lanegcn.py:696-699):
 *   out[j] = x W_j^T   for j < n_w, n_w = 1 or 2
 * in ONE weight-stationary launch: a workgroup reads a 48-row tile of x once, each of its 8 waves keeps a 32-channel
 * slice of one weight in registers over the full K, and the results are stored straight from the accumulators.
 *   x, out[j]: fp32 [n_rows,128];  w[j]: lgcn_pack_weight image (k = 128) of W_j for `mma`;  w, out: HOST arrays of n_w
 *   device pointers.
 * Bit-identical to lgcn_agg_mlp with one LGCN_REL_IDENT relation (src = x, wp = w[j]) and flags = 0: same operand roles,
 * one fp32 accumulator per element, K-steps and plane products in the same order.
 * LGCN_MMA_F16X2 and LGCN_MMA_BF16 only (others: LGCN_ESHAPE, checked first -- use lgcn_agg_mlp there).  n_rows < 0, n_w
 * outside 1..2, a NULL array or, with n_rows > 0, a NULL x / w[j] / out[j]: LGCN_EINVAL; n_rows > 2^31 - 1: LGCN_ESHAPE;
 * pointers not 16-byte aligned: LGCN_EALIGN.  n_rows == 0 returns LGCN_OK without a launch.
 */
int lgcn_ctx_heads(const float *x, int64_t n_rows, const void *const *w, int n_w, int mma, float *const *out, void *stream);

/*
 * Node-side tail of an Att block whose targets outnumber its context rows (A2M: the lane nodes; lanegcn.py:702-709),
 * weight-stationary: the lgcn_agg_mlp problem
 *   rel = {LGCN_REL_IDENT(a, W_agt), LGCN_REL_RANGE(m, W_c1)} with rowptr [N+1], flags = GN1 | RELU1 | GEMM2 | GN2 | RES |
 *   RELU2, gn1, wp2, gn2, res, out, and optionally the chained U output (ch_wq, ch_gq_*, ch_wu, ch_u_out)
 * on 48-row tiles whose 8 waves each keep a 16-channel slice of every weight in registers over the full K, each slice
 * requested a GEMM or more before it is used.  Bit-identical to lgcn_agg_mlp on the same problem: the same accumulation
 * order (relation 0 then 1, K-steps and plane products in order), the same GroupNorm sums, the segment sum in pair order.
 * Exactly that shape: LGCN_MMA_F32 / LGCN_MMA_BF16X3 (checked first), any other relation list or flags, a chained V
 * output, w4, out_pre / out_mid / out_pre2 or a tile_rb: LGCN_ESHAPE -- use lgcn_agg_mlp there.  n_rows < 0 or a NULL
 * required pointer: LGCN_EINVAL; n_rows > 2^31 - 1: LGCN_ESHAPE; pointers (but rowptr) not 16-byte aligned: LGCN_EALIGN.
 * n_rows == 0 returns LGCN_OK without a launch.
 */
int lgcn_node_tail(const lgcn_agg_mlp_t *p_host, void *stream);

/*
 * Head of an Att block whose targets are the lane nodes (A2M's first launch; lanegcn.py:387-406, 696-699),
 * weight-stationary: 1 <= n <= LGCN_MAX_MULTI lgcn_agg_mlp problems of one LGCN_REL_IDENT relation each in ONE launch, on
 * 48-row tiles whose 8 waves each keep a 16-channel slice of every weight in registers over the full K.  A problem is a
 *   head   : flags = GN1 | RELU1, gn1, out, optionally the rank-4 update (w4, x4_*) and the chained U output (ch_wq,
 *            ch_gq_*, ch_wu, ch_u_out);
 *   u-chain: flags = GN1 | RELU1 | GEMM2, gn1, wp2, out;
 *   plain  : flags = 0, out.
 * Problems with the same src and n_rows, the head apart, share their tiles (the rows are read once): up to two plain ones
 * and a u-chain per tile range.
 * Bit-identical to lgcn_agg_mlp_multi on the same problems: one fp32 accumulator per element, K-steps and plane products
 * in the same order, the same rank-4 arithmetic and GroupNorm sums.
 * LGCN_MMA_F32 / LGCN_MMA_BF16X3 or problems of different modes (checked first), any other relation list or flags, a
 * chained V output, w4 or a chained U outside a head, out_pre / out_mid / out_pre2 or a tile_rb: LGCN_ESHAPE -- use
 * lgcn_agg_mlp_multi there.  n out of range, a NULL problem, n_rows < 0 or a NULL required pointer: LGCN_EINVAL; n_rows >
 * 2^31 - 1: LGCN_ESHAPE; pointers (but x4_*) not 16-byte aligned: LGCN_EALIGN.  A problem with n_rows == 0 adds no tiles
 * and its pointers are not looked at; if every problem is empty the call returns LGCN_OK without a launch.
 */
int lgcn_node_head(const lgcn_agg_mlp_t *const *ps_host, int n, void *stream);

/*
 * MapNet input stage, lanegcn.py:324-327:
 *   out = ReLU( GN_a(W_a2 ReLU(W_a1 ctr + b_a1)) + GN_s(W_s2 ReLU(W_s1 seg + b_s1)) )
 * ctrs, feats: [N,2]; w1: [128,2] + b1 [128] (nn.Linear(2,128)); wp2: packed.
 */
int lgcn_mapnet_input(const float *ctrs, const float *feats, int64_t n_rows,
                      const float *wa1, const float *ba1, const float *wpa2,
                      const float *ga, const float *bta,
                      const float *ws1, const float *bs1, const float *wps2,
                      const float *gs, const float *bts,
                      float eps, int mma, float *out, void *stream);

/*
 * Att.forward per-pair MLP, lanegcn.py:691-700, for pairs p < *n_pairs:
 *   d   = agt_ctrs[hi[p]] - ctx_ctrs[wi[p]]
 *   e   = ReLU(GN_d(W_d2 ReLU(W_d0 d + b_d0)))
 *   m_p = ReLU(GN_c( W_c0[:, 0:128] e + U[hi[p]] + V[wi[p]] ))
 * where U = query(agts) W_c0[:,128:256]^T (per target row) and
 * V = ctx W_c0[:,256:384]^T (per context row) were hoisted out of the pair
 * loop (row-wise Linear commutes with the gather).  ctx.1 (:654) is applied
 * after the segment sum by lgcn_agg_mlp (it is linear).
 * m: [cap,128] output rows.  LGCN_MMA_F32 only (others: LGCN_ESHAPE -- use lgcn_att_pairs_ws / lgcn_att_pairs_wi).
 */
int lgcn_att_pairs(const float *agt_ctrs, const float *ctx_ctrs,
                   const int32_t *hi, const int32_t *wi,
                   const int32_t *n_pairs, int64_t cap,
                   const float *wd0, const float *bd0, const float *wpd2,
                   const float *gd, const float *btd,
                   const float *wpc0e, const float *U, const float *V,
                   const float *gc, const float *btc,
                   float eps, int mma, float *m, void *stream);

/*
 * The m_p of lgcn_att_pairs in the split-precision modes, with both 128 x 128 weights held in registers by persistent
 * workgroups (64-pair tiles) instead of streamed through the CU per tile.  Split-precision modes only (F32: LGCN_ESHAPE).
 *   seg = 0 : m[p] = m_p for every pair p < *n_pairs (as lgcn_att_pairs).
 *   seg = 16: hi must be sorted (lgcn_pairs_build output).  Within every 16-aligned group of pair rows the rows of
 *             one target are summed in pair order; the sum is written at the row of the piece's first pair and the
 *             other rows of m are left untouched.  Pass m to lgcn_agg_mlp as an LGCN_REL_RANGE16 relation: for few
 *             targets with many pairs each (M2A, A2A) the tail then reads ~1/12 of the rows.
 */
int lgcn_att_pairs_ws(const float *agt_ctrs, const float *ctx_ctrs,
                      const int32_t *hi, const int32_t *wi,
                      const int32_t *n_pairs, int64_t cap,
                      const float *wd0, const float *bd0, const float *wpd2,
                      const float *gd, const float *btd,
                      const float *wpc0e, const float *U, const float *V,
                      const float *gc, const float *btc,
                      float eps, int mma, int seg, float *m, void *stream);

/*
 * lgcn_att_pairs_ws with WAVE-INDEPENDENT 16-pair blocks (csrc/lgcn_pairs.hip): the weights in LDS one at a time (W_d2,
 * then W_c0e after a workgroup barrier; 8-wave workgroups), a wave takes 16 pair rows from the centre offsets to m,
 * meeting the other waves only at the weight copies; GroupNorm / ReLU / plane split
 * in registers (the accumulator layout of one GEMM is the operand layout of the next, thanks to a K permutation of
 * the weights).  Same outputs as lgcn_att_pairs_ws (seg = 0 / 16) up to fp32 summation order.
 *   wkd2, wkc0e: images of Att.dist.2's Linear weight and of ctx.0's columns 0..127 made by lgcn_pack_weight_kperm
 *   (2 x 32 KiB in F16X2, 32 KiB in BF16).  LGCN_MMA_F16X2 and LGCN_MMA_BF16 only (others: LGCN_ESHAPE; use
 *   lgcn_att_pairs_ws).  U and V rows are addressed with 32-bit byte
 *   offsets: fewer than 2^23 target / context rows.
 */
int lgcn_pack_weight_kperm(const float *W, int ld, int mma, void *out, void *stream);
int lgcn_att_pairs_wi(const float *agt_ctrs, const float *ctx_ctrs,
                      const int32_t *hi, const int32_t *wi,
                      const int32_t *n_pairs, int64_t cap,
                      const float *wd0, const float *bd0, const float *wkd2,
                      const float *gd, const float *btd,
                      const float *wkc0e, const float *U, const float *V,
                      const float *gc, const float *btc,
                      float eps, int mma, int seg, float *m, void *stream);

/*
 * Training of the pair stage of Att (reference lanegcn.py:691-703), exact fp32 whatever the matrix mode of the rest
 * of the network.  Per pair p < *n_pairs (clamped to cap), h = hi[p], w = wi[p]:
 *   d  = agt_ctrs[h] - ctx_ctrs[w]
 *   z0 = W_d0 d + b_d0;                    h1 = ReLU(z0)         mask0 = z0 > 0
 *   t1 = W_d2 h1;                          e  = ReLU(GN_d(t1))   mask1 = e  > 0
 *   c  = W_c0[:, 0:128] e + U[h] + V[w];   m  = ReLU(GN_c(c))    mask2 = m  > 0
 * and S[t] = sum of m_p over the pairs of target t (lgcn_gather_sum over the pair search's rowptr).
 *
 * lgcn_att_pairs_train: lgcn_att_pairs (LGCN_MMA_F32 images wpd2, wpc0e) with one more output, the three masks as bits;
 * m is bit for bit what lgcn_att_pairs writes.
 *   masks: [cap, 3, 4] uint32, rows < *n_pairs written: masks[p][k][j] bit b = mask k of channel 32 j + b.
 *
 * lgcn_att_pairs_bwd, for dS [T,128] (one main launch + one fixed-order reduction launch; no atomics, no host read):
 *   g2 = dS[h] * mask2;  dgamma_c += g2 * chat;  dbeta_c += g2;  dc = GN_c backward of g2 (formula of lgcn_gn_bwd)
 *   dW_c0[:, 0:128] += dc (x) e;  de = dc W_c0[:, 0:128]
 *   g1 = de * mask1;  dgamma_d += g1 * t1hat;  dbeta_d += g1;  dt1 = GN_d backward of g1
 *   dW_d2 += dt1 (x) h1;  dh1 = dt1 W_d2;  dz0 = dh1 * mask0;  dW_d0 += dz0 (x) d;  db_d0 += dz0
 * h1, t1, e, c and the GroupNorm statistics are recomputed per 32-pair tile with the forward's device functions; the
 * masks are read, not re-derived.  dU[h] += dc and dV[w] += dc are lgcn_gather_sum launches over dc (by the pair
 * search's rowptr, and by a CSR of the pairs by context row).
 *   wptd2, wptc0e: lgcn_pack_weight_t images (LGCN_MMA_F32) of W_d2 and of W_c0[:, 0:128]
 *   dc:     [cap,128], rows < *n_pairs written -- the only per-pair tensor that reaches memory; may be NULL
 *   d_*:    gradient outputs, each may be NULL and its work is then skipped: d_wd2, d_wc0e [128,128] (d_wc0e is the
 *           dense [128,128] block of columns 0:128), d_wd0 [128,2], d_bd0, d_gd, d_btd, d_gc, d_btc [128]
 *   n_chunks: 1..1024 workgroups (never more than ceil(cap / 32) are launched): workgroup k owns the tiles k,
 *           k + n_chunks, ... and writes one record of 2 * 128 * 128 + 7 * 128 floats -- dW_d2, dW_c0e, dgamma_c,
 *           dbeta_c, dgamma_d, dbeta_d, db_d0, dW_d0[:,0], dW_d0[:,1]; the second launch sums the records in chunk order.
 *   ws:     lgcn_att_pairs_bwd_ws_elems(cap, n_chunks) floats (negative: LGCN_EINVAL for cap < 0, cap too large or
 *           n_chunks outside 1..1024); needed when any d_* is given.
 */
typedef struct {
    const float *agt_ctrs, *ctx_ctrs;
    const int32_t *hi, *wi, *n_pairs;
    int64_t cap;
    const float *wd0, *bd0, *wpd2, *gd, *btd, *wpc0e, *U, *V, *gc, *btc;
    const float *wptd2, *wptc0e;
    const uint32_t *masks;
    const float *dS;
    float *dc, *d_wd2, *d_wc0e, *d_wd0, *d_bd0, *d_gd, *d_btd, *d_gc, *d_btc, *ws;
    float eps;
    int32_t n_chunks;
} lgcn_att_pairs_bwd_t;

int lgcn_att_pairs_train(const float *agt_ctrs, const float *ctx_ctrs,
                         const int32_t *hi, const int32_t *wi,
                         const int32_t *n_pairs, int64_t cap,
                         const float *wd0, const float *bd0, const float *wpd2,
                         const float *gd, const float *btd,
                         const float *wpc0e, const float *U, const float *V,
                         const float *gc, const float *btc,
                         float eps, float *m, uint32_t *masks, void *stream);
int64_t lgcn_att_pairs_bwd_ws_elems(int64_t cap, int n_chunks);
int lgcn_att_pairs_bwd(const lgcn_att_pairs_bwd_t *p_host, void *stream);

/*
 * The pair stage of the fork's LanePooling (reference lanercnn.py:492-499) in one launch, exact fp32 whatever the matrix
 * mode of the rest of the network.  Per pair p < *n_pairs (a negative or larger count is clamped to cap, as in
 * lgcn_att_pairs), t = ti[p] the target row and c = ci[p] the context row:
 *   d    = ctx_pose[c] - tgt_pose[t]                 4 floats, one fp32 subtraction each (:494)
 *   h    = ReLU(W_p d + b_p)                         relpose.0 (:495)
 *   z    = W_0[:, 128:256] h + U[c]                  ctx.0's Linear over cat(context feature, h) (:497-499)
 *   m[p] = ReLU(GN(z; g, bt, eps))                   ctx.0's GroupNorm(1,128) and ReLU
 * where U = context_feat W_0[:, 0:128]^T (one row per context row) was hoisted out of the pair loop.  ctx.1 (linear) is
 * applied after the per-target segment sum by lgcn_agg_mlp (an LGCN_REL_RANGE relation over m).
 *   ctx_pose [C,4], tgt_pose [T,4]: rows of 16 bytes, 16-byte aligned; ti, ci: [cap] int32
 *   wp [128,4], bp [128]: relpose.0; wpc0h: lgcn_pack_weight image (LGCN_MMA_F32) of ctx.0's columns 128:256
 *   m: [cap,128]; only rows < the count are written.  No atomics, no workspace: results are bitwise repeatable.
 * NULL pointers and cap < 0: LGCN_EINVAL; misaligned pointers: LGCN_EALIGN; cap > 0x7ffffff0: LGCN_ESHAPE; cap == 0
 * returns LGCN_OK without a launch.
 */
int lgcn_pool_pairs(const float *ctx_pose, const float *tgt_pose,
                    const int32_t *ti, const int32_t *ci,
                    const int32_t *n_pairs, int64_t cap,
                    const float *wp, const float *bp, const float *wpc0h,
                    const float *U, const float *g, const float *bt,
                    float eps, float *m, void *stream);

/*
 * Training of the pair stage of LanePooling, exact fp32 whatever the matrix mode of the rest of the network.  Notation of
 * lgcn_pool_pairs: per pair p < *n_pairs (clamped to cap), t = ti[p], c = ci[p], d = ctx_pose[c] - tgt_pose[t]:
 *   y0 = W_p d + b_p;             h = ReLU(y0)          mask0 = y0 > 0
 *   z  = W_0[:, 128:256] h + U[c]
 *   m  = ReLU(GN(z; g, bt))                             mask1 = m  > 0
 * and S[t] = sum of m_p over the pairs of target t (lgcn_gather_sum over the pair search's rowptr).
 *
 * lgcn_pool_pairs_train: lgcn_pool_pairs with one more output, the two masks as bits; m is bit for bit what
 * lgcn_pool_pairs writes.
 *   masks: [cap, 2, 4] uint32, rows < *n_pairs written: masks[p][k][j] bit b = mask k of channel 32 j + b (the layout of
 *           lgcn_att_pairs_train), 32 bytes per pair.
 *
 * lgcn_pool_pairs_bwd, for dS [T,128] (one main launch + one fixed-order reduction launch; no atomics, no host read):
 *   g  = dS[t] * mask1;  dgamma += g * zhat;  dbeta += g;  dz = GN backward of g (formula of lgcn_gn_bwd)
 *   dW_0[:, 128:256] += dz (x) h;  dh = dz W_0[:, 128:256]
 *   dy0 = dh * mask0;  dW_p += dy0 (x) d  ([128,4]);  db_p += dy0
 * h, z and the GroupNorm statistics are recomputed per 32-pair tile with the forward's device functions; the masks are
 * read, not re-derived.  dU[c] += dz is an lgcn_gather_sum launch over dz by a CSR of the pairs by context row.  The
 * poses get no gradient.
 *   wptc0h: lgcn_pack_weight_t image (LGCN_MMA_F32) of W_0[:, 128:256]; needed when d_wp or d_bp is given
 *   dz:     [cap,128], rows < *n_pairs written -- the only per-pair tensor that reaches memory; may be NULL
 *   d_*:    gradient outputs, each may be NULL and its work is then skipped: d_w0h [128,128] (the dense block of columns
 *           128:256), d_wp [128,4], d_bp, d_g, d_bt [128].  With none of them the launch stops after the GroupNorm
 *           backward; without d_wp and d_bp it skips the dh GEMM.
 *   n_chunks: 1..1024 workgroups (never more than ceil(cap / 32) are launched): workgroup k owns the tiles k,
 *           k + n_chunks, ... and writes one record of 128 * 128 + 7 * 128 floats -- dW_0h, dgamma, dbeta, db_p,
 *           dW_p[:,0..3]; the second launch sums the records in chunk order.
 *   ws:     lgcn_pool_pairs_bwd_ws_elems(cap, n_chunks) floats (negative: LGCN_EINVAL for cap < 0, cap too large or
 *           n_chunks outside 1..1024); needed when any d_* is given.
 * NULL required pointers, cap < 0, n_chunks outside 1..1024, a missing ws: LGCN_EINVAL; misaligned pointers: LGCN_EALIGN;
 * cap > 0x7ffffff0: LGCN_ESHAPE; cap == 0 returns LGCN_OK without a launch.  All decided before anything is launched.
 */
typedef struct {
    const float *ctx_pose, *tgt_pose;
    const int32_t *ti, *ci, *n_pairs;
    int64_t cap;
    const float *wp, *bp, *wpc0h, *U, *g, *bt;
    const float *wptc0h;
    const uint32_t *masks;
    const float *dS;
    float *dz, *d_w0h, *d_wp, *d_bp, *d_g, *d_bt, *ws;
    float eps;
    int32_t n_chunks;
} lgcn_pool_pairs_bwd_t;

int lgcn_pool_pairs_train(const float *ctx_pose, const float *tgt_pose,
                          const int32_t *ti, const int32_t *ci,
                          const int32_t *n_pairs, int64_t cap,
                          const float *wp, const float *bp, const float *wpc0h,
                          const float *U, const float *g, const float *bt,
                          float eps, float *m, uint32_t *masks, void *stream);
int64_t lgcn_pool_pairs_bwd_ws_elems(int64_t cap, int n_chunks);
int lgcn_pool_pairs_bwd(const lgcn_pool_pairs_bwd_t *p_host, void *stream);

/*
 * PredLoss (reference lanegcn.py:740-807), forward and backward, one launch each.
 *   cls [A, M], reg [A, M, T, 2], gt [A, T, 2] fp32; has [A, T] bytes (torch.bool); M <= 8, T <= 64.
 * Per actor: last = argmax_t(has[t] + 0.1 t / T), kept iff that maximum > 1.0; dist_j = |reg[j, last] - gt[last]|;
 * (min_dist, min_idx) = min_j; max-margin term over the modes j with min_dist < cls_th and dist_j - min_dist >
 * cls_ignore and cls[min_idx] - cls[j] < mgn; SmoothL1 (beta 1) of reg[min_idx, t] - gt[t] over the observed steps.
 *   sums[0] = cls_coef * sum (mgn - margin), sums[1] = reg_coef * sum SmoothL1; counts[0] = num_cls, counts[1] = num_reg
 *   (the reference's loss_out entries; Loss.forward divides by the counts, :818-820);
 *   sel [A]: min_idx | (hinge bits << 8), -1 for a dropped actor: input of the backward.
 * Index / mask decisions use the same fp32 operations as ATen; sums in a fixed order (no atomics).
 * Backward: dcls [A, M], dreg [A, M, T, 2] (every element written) for upstream gradients g_cls, g_reg (device scalars).
 */
int lgcn_pred_loss_fwd(const float *cls, const float *reg, const float *gt, const unsigned char *has, int64_t n_act,
                       int n_mod, int n_t, float cls_th, float cls_ignore, float mgn, float cls_coef, float reg_coef,
                       float *sums, int32_t *counts, int32_t *sel, void *stream);
int lgcn_pred_loss_bwd(const float *cls, const float *reg, const float *gt, const unsigned char *has, int64_t n_act,
                       int n_mod, int n_t, float cls_coef, float reg_coef, const int32_t *sel, const float *g_cls,
                       const float *g_reg, float *dcls, float *dreg, void *stream);

/* ------------------------------------------------------------------ */
/* Backward building blocks (fp32; the row-GEMMs of the backward are     */
/* lgcn_agg_mlp launches on transposed plans / transposed weights)       */
/* ------------------------------------------------------------------ */

/*
 * Backward of  y = [ReLU]( GroupNorm(1,128)(x) [+ res] )  for row-major [n_rows,128] tensors
 * (layers.py:73-87 and the norm/relu/residual lines of lanegcn.py:356-361, 704-709):
 *   g  = dy * (post > 0)            when post != NULL (post = the forward output after ReLU)
 *   dx = rstd * (g*gamma - mean(g*gamma) - xhat * mean(g*gamma*xhat)),  xhat = (x - mean) * rstd
 *   dgamma = sum_rows g * xhat,  dbeta = sum_rows g
 * dg_out (optional, [n_rows,128]) receives g itself (the gradient that flows into `res`).
 * gamma == NULL: no normalisation (dx = g), used for plain ReLU masks.
 * dgamma / dbeta: [128] outputs; part: workspace of 2 * ceil(n_rows/32) * 128 floats.
 * Deterministic (two-level tree, no atomics).
 * Statistics: mean in two steps (the fp32 mean, then the mean of the centred values: a row at 2^10 with a spread of 1 keeps
 * xhat at fp32 rounding), and rows whose fp32 sum of squares overflows (beyond ~2^60) take the forward's wide path: rstd
 * from the centred values scaled by 2^-68, so forward and backward agree on such rows (dx ~ rstd dy stays inside fp32).
 * The same holds for the recomputations inside lgcn_laneconv_bwd, lgcn_rowblock_bwd and lgcn_att_pairs_bwd; a row in which
 * two such norms meet (laneconv: T and Z both beyond 2^60) has gradients ~ 2^-140 that leave fp32 by themselves.
 * lgcn_gn_cl_bwd and lgcn_conv1d_gn_bwd take the two-step mean only (their forward has no wide path).
 */
int lgcn_gn_bwd(const float *dy, const float *x, const float *post, const float *gamma,
                int64_t n_rows, float eps, float *dx, float *dg_out,
                float *dgamma, float *dbeta, float *part, void *stream);

/*
 * Weight gradients of an aggregate-GEMM stage T = sum_r (G_r src_r) W_r^T:
 *   dW[r] = dT^T (G_r src_r)      [128,128] per relation, fp32 (f32-input MFMA, exact fma chain)
 * The relations (src, mode, ridx), rowptr/col/n_rel_csr and n_rows are read from *p exactly as
 * lgcn_agg_mlp reads them (wp and the epilogue fields are ignored).
 * dW: [n_rel,128,128]; part: workspace of n_rel * n_chunks * 128*128 floats, n_chunks in 1..1024 (pick n_rel * n_chunks ~ 2 workgroups per CU).
 */
int lgcn_wgrad(const lgcn_agg_mlp_t *p_host, const float *dT, float *dW, float *part,
               int n_chunks, void *stream);

/*
 * Backward of one LaneConv / LinearRes block (reference lanegcn.py:331-362, layers.py:193-238) below its aggregate stage,
 * exact fp32 whatever the matrix mode of the rest of the network.  The forward (lgcn_agg_mlp with every epilogue flag and
 * out_pre = T, out_mid = Y, out_pre2 = Z) computed, per row,
 *   T = sum_r (G_r X) W_r^T;   Y = ReLU(GN1(T));   Z = Y W2^T;   out = ReLU(GN2(Z) + X)
 * lgcn_laneconv_bwd, for d_out [n_rows,128] (one main launch + one fixed-order reduction launch; no atomics, no host read):
 *   g2 = d_out * (out > 0);  dgamma2 += g2 * zhat;  dbeta2 += g2;  dZ = GN2 backward of g2 (formula of lgcn_gn_bwd)
 *   dW2 += dZ (x) Y;  dY = dZ W2
 *   g1 = dY * (Y > 0);  dgamma1 += g1 * that;  dbeta1 += g1;  dT = GN1 backward of g1
 * zhat, that and the GroupNorm statistics are recomputed per 32-row tile from the saved Z and T.
 * ident1 == 0 (any relations): dT and g2 are written, rows < n_rows only; the caller finishes with the launches it already
 *   has: dX = sum_r G_r^T dT W_r + g2 (lgcn_agg_mlp on the transposed plan, LGCN_F_RES with res = g2) and dW_r (lgcn_wgrad).
 * ident1 == 1 (T = X W1^T, one IDENT relation): the entry finishes the block,
 *   dX = dT W1 + g2;  dW1 += dT (x) X
 *   and neither dT nor g2 reaches memory.
 *   d_out, out, Z, Y, T: [n_rows,128]; X: [n_rows,128], ident1 only;  gamma1, gamma2: the GroupNorm weights [128]
 *   wpt2, wpt1: lgcn_pack_weight_t images (LGCN_MMA_F32) of W2 and, ident1 only, of W1
 *   dT, g2: [n_rows,128] outputs of ident1 == 0, each may be NULL (no g2: no dX is wanted)
 *   dX:     [n_rows,128] output of ident1 == 1, may be NULL (its GEMM is then skipped)
 *   d_*:    gradient outputs, each may be NULL and its work is then skipped: d_w2 [128,128], d_w1 [128,128] (ident1 only),
 *           d_g2, d_b2, d_g1, d_b1 [128].  An output of the other variant (dX / d_w1 with ident1 == 0, dT / g2 with
 *           ident1 == 1) is LGCN_EINVAL.
 *   n_chunks: 1..1024 workgroups (never more than ceil(n_rows / 32) are launched): workgroup k owns the tiles k,
 *           k + n_chunks, ... and writes one record of (1 + ident1) * 128 * 128 + 4 * 128 floats -- dW2, dW1 (ident1 only),
 *           dgamma2, dbeta2, dgamma1, dbeta1; the second launch sums the records in chunk order.
 *   ws:     lgcn_laneconv_bwd_ws_elems(n_rows, n_chunks, ident1) floats (negative: LGCN_EINVAL for n_rows < 0 or above
 *           0x7fffffff, n_chunks outside 1..1024 or ident1 outside 0..1); needed when any d_* is given.
 * n_rows == 0, or every output NULL: LGCN_OK without a launch.
 */
typedef struct {
    const float *d_out, *out, *Z, *Y, *T, *X;
    const float *gamma1, *gamma2, *wpt2, *wpt1;
    float *dT, *g2, *dX;
    float *d_w2, *d_w1, *d_g2, *d_b2, *d_g1, *d_b1, *ws;
    int64_t n_rows;
    float eps;
    int32_t n_chunks, ident1, pad_;
} lgcn_laneconv_bwd_t;

int64_t lgcn_laneconv_bwd_ws_elems(int64_t n_rows, int n_chunks, int ident1);
int lgcn_laneconv_bwd(const lgcn_laneconv_bwd_t *p_host, void *stream);

/*
 * Backward of one row block with IDENT relations only,
 *   out = [ReLU]( [GN]( sum_{r < n_rel} src_r W_r^T ) [+ res] )       (lgcn_agg_mlp with out_pre = `pre`),
 * exact fp32 whatever the matrix mode of the rest of the network: the backward of layers.Linear, the input stems' second
 * layers, A2M's meta layer, AttDest and the node side of Att.  For d_out [n_rows,128] (one main launch + one fixed-order
 * reduction launch; no atomics, no host read):
 *   g     = d_out * (out > 0)         when out != NULL (the block had a ReLU), else d_out
 *   d_res = g                         written only when d_res != NULL (a caller asks only when there was a ReLU and a residual;
 *                                     without a ReLU the gradient of the residual is d_out itself)
 *   no GN (pre == gamma == NULL):  dT = g
 *   GN:   xhat, rstd recomputed per 32-row tile from the saved `pre`;  dT = GN backward of g (formula of lgcn_gn_bwd);
 *         dgamma += g * xhat;  dbeta += g
 *   for r < n_rel (1 or 2):   d_src[r] = dT W_r        (on wpt[r], the lgcn_pack_weight_t LGCN_MMA_F32 image of the 128 x 128 block)
 *                             d_w[r]  += dT (x) src_r  (v_mfma_f32_32x32x2_f32), written with row stride ld_w[r]
 *   d_out, out, pre, src[r], d_src[r], d_res: [n_rows,128];  gamma, d_gamma, d_beta: [128]
 *   src[r], wpt[r]: required for r < n_rel;  pre and gamma: both or neither;  d_gamma / d_beta without them: LGCN_EINVAL
 *   d_src[r], d_w[r], d_res, d_gamma, d_beta: each may be NULL and its work is then skipped.  Rows >= n_rows of d_src[r] /
 *           d_res are never written.
 *   d_w[r]: the [128,128] block at columns col0 .. col0 + 128 of a row-major [128,K] gradient: the pointer to element
 *           (0, col0), ld_w[r] = K floats (>= 128, a multiple of 4; 16-byte alignment asks the same of col0).  Only the
 *           block is written; two relations may name two blocks of one gradient.
 *   n_chunks: 1..1024 workgroups (never more than ceil(n_rows / 32) are launched): workgroup k owns the tiles k,
 *           k + n_chunks, ... and writes one record of n_rel * 128 * 128 + 2 * 128 floats -- dW_0, dW_1 (two relations
 *           only), dgamma, dbeta; the second launch sums the records in chunk order into the outputs asked for.
 *   ws:     lgcn_rowblock_bwd_ws_elems(n_rows, n_chunks, n_rel) floats (negative: LGCN_EINVAL for n_rows < 0 or above
 *           0x7fffffff, n_chunks outside 1..1024 or n_rel outside 1..2); needed when any of d_w[r], d_gamma, d_beta is
 *           given.  Without one of them there is no record and no second launch.
 * Checked before anything is launched, in this order: the struct, n_rows (negative: LGCN_EINVAL, above 0x7fffffff:
 * LGCN_ESHAPE), n_rel, n_chunks, the required pointers, ld_w, then 16-byte alignment of every pointer (LGCN_EALIGN; those of
 * an unused second relation included).  n_rows == 0, or every output NULL: LGCN_OK without a launch.
 */
typedef struct {
    const float *d_out, *out, *pre, *gamma;
    const float *src[2], *wpt[2];
    float *d_src[2], *d_w[2];
    float *d_res, *d_gamma, *d_beta, *ws;
    int64_t n_rows;
    int32_t ld_w[2];
    float eps;
    int32_t n_rel, n_chunks, pad_;
} lgcn_rowblock_bwd_t;

int64_t lgcn_rowblock_bwd_ws_elems(int64_t n_rows, int n_chunks, int n_rel);
int lgcn_rowblock_bwd(const lgcn_rowblock_bwd_t *p_host, void *stream);

/*
 * Forward of  out = [ReLU]( GroupNorm(1,128)(x) [+ res] )  as a stand-alone row kernel (the fused
 * kernels do this in their epilogues; the differentiable per-pair composition needs it alone).
 * gamma == NULL: no normalisation.  relu != 0 applies the ReLU.
 */
int lgcn_gn_fwd(const float *x, const float *gamma, const float *beta, const float *res,
                int64_t n_rows, float eps, int relu, float *out, void *stream);

/*
 * GroupNorm with ONE group over the C x L elements of every item of x [n_items, C, L] (contiguous: channel
 * c = element / L), per-channel gamma / beta, then optional "+ res" (same shape) and ReLU, in one launch:
 *   out = [ReLU]( (x - mean_item) * rstd_item * gamma[c] + beta[c] [+ res] )
 * This is ActorNet's Conv1d / Res1d norm (reference layers.py:40-62, 142-190 with ng = 1; biased variance,
 * two-pass), which stock ATen runs as three to five launches per call.  C * L <= 16384.
 * res_up2 != 0: res is [n_items, C, L/2] (L even) and is upsampled x2 on the fly (linear, align_corners = False:
 * res'[2i] = 0.25 r[i-1] + 0.75 r[i], res'[2i+1] = 0.75 r[i] + 0.25 r[i+1], edges clamped) -- the top-down step of
 * the FPN, "interpolate(out, scale_factor=2, mode='linear') + lateral(x)", reference lanegcn.py:256-260.
 * channels_last != 0: x, res and out are stored [n_items, L, C] (element = l * C + c), the layout in which MIOpen's
 * convolutions run without transposes (torch.channels_last on [n, C, 1, L]).
 */
int lgcn_gn_cl(const float *x, int64_t n_items, int C, int L, const float *gamma, const float *beta,
               float eps, const float *res, int res_up2, int relu, int channels_last, float *out, void *stream);

/*
 * Backward of lgcn_gn_cl (layout [n_items, C, L], channels_last = 0):  given dy and the forward's x (and its
 * output `post` when a ReLU was applied: the mask is post > 0),
 *   g   = dy masked                      (also the gradient into res; written when g != NULL)
 *   dx  = rstd * (g gamma - mean_item(g gamma) - xhat * mean_item(g gamma xhat))
 *   part[item][0][c] = sum_l g xhat,  part[item][1][c] = sum_l g     (dgamma / dbeta = column sums over items)
 * part: [n_items, 2, C] floats.  No atomics: the caller sums `part` over items.
 */
int lgcn_gn_cl_bwd(const float *dy, const float *x, const float *post, const float *gamma, int64_t n_items,
                   int C, int L, float eps, float *dx, float *g, float *part, void *stream);

/*
 * out[n] = sum_{j in [rowptr[n], rowptr[n+1])} src[col ? col[j] : j]   for n < n_rows (rows of 128 floats,
 * fixed summation order).  col == NULL: contiguous segments (index_add_ by a sorted index, lanegcn.py:703);
 * with col: a plain CSR (transposes of gathers in the backward).
 */
int lgcn_gather_sum(const float *src, const int32_t *rowptr, const int32_t *col, int64_t n_rows,
                    float *out, void *stream);

/* out[p] = c[p] + U[hi[p]] + V[wi[p]] for p < *n (device count, clamped to cap)  (lanegcn.py:696-699 after
 * hoisting the row-wise Linears out of the pair loop). */
int lgcn_pair_add(const float *c, const float *U, const int32_t *hi, const float *V, const int32_t *wi,
                  const int32_t *n_dev, int64_t cap, float *out, void *stream);

/* out[i] = src[idx[i]] for i < *n (device count, clamped to cap); rows of 128 floats. */
int lgcn_gather_rows(const float *src, const int32_t *idx, const int32_t *n_dev, int64_t cap,
                     float *out, void *stream);

/*
 * Range check of the 16-bit-plane matrix modes.  LGCN_MMA_F16X2 operands must stay below 65520, the first value that rounds
 * to fp16's infinity (BF16X3 / BF16: bf16's 3.4e38); an operand from there on becomes +-inf planes, whose products cancel to NaN, and every ReLU of this
 * library keeps a NaN a NaN (like ATen's), so the row it belongs to -- and every row fed by it -- reaches the stage
 * output as NaN rather than as plausible numbers.  lgcn_check_finite looks for that on the device:
 *   flag[0] |= bit  if any of a[0..na) or b[0..nb) is not finite   (a, b 16-byte aligned; flag zeroed by the caller).
 * The host side reads the flag once per forward and re-runs a flagged forward in LGCN_MMA_BF16X3 (ops.py: guarded).
 */
int lgcn_check_finite(const float *a, int64_t na, const float *b, int64_t nb, int32_t *flag, int bit, void *stream);
/*
 * The same check over the REAL rows of a padded batch (lgcn_store_gather_pad): a holds na / row_a rows of row_a floats,
 * of which the first rows_a[0] are looked at (rows_a: one int64 on the device, read by the kernel and clamped to
 * [0, na / row_a]); b, nb, row_b, rows_b likewise.  The grid depends on na + nb alone, so the launch is the same for
 * every batch of one capacity.  LGCN_EINVAL: a negative size, bit 0, a NULL pointer next to a non-zero size, a row
 * length that is not positive or does not divide its size; LGCN_EALIGN: a, b not 16-byte, rows_a, rows_b not 8-byte aligned.
 */
int lgcn_check_finite_rows(const float *a, int64_t na, int64_t row_a, const int64_t *rows_a, const float *b, int64_t nb,
                           int64_t row_b, const int64_t *rows_b, int32_t *flag, int bit, void *stream);

/*
 * Exact-fp32 form of lgcn_conv1d_gn / lgcn_conv1d_gn_train (reference layers.py:40-62 Conv1d, 142-190 the halves of Res1d;
 * ActorNet lanegcn.py:212-263): the same unit, shape set, residual modes, workgroups of whole actors and GroupNorm epilogue,
 * with fp32 operands on v_mfma_f32_16x16x4_f32 instead of two fp16 planes.  No operand range limit; one fused
 * multiply-add chain per output in a fixed order (taps outer, 32-channel chunks, 4 channels of each K quarter), no
 * atomics: bitwise repeatable, and independent of any matrix mode.
 * wp: lgcn_conv_pack_weight_f32 image of W [cout, cin, ks] (lgcn_conv_packed_f32_bytes bytes; per tap, 32-channel chunk
 * and 16-output block two 64 x 16-byte fragments: lane (n, kq) holds W[16 cb + n][32 kc + 16 h + 4 kq + 0..3][t];
 * channels beyond cin are zero).  y == NULL: inference; otherwise y [A, lout, cout] receives the pre-norm convolution
 * output as lgcn_conv1d_gn_train stores it, which lgcn_conv1d_gn_bwd consumes unchanged (y must be 16-byte aligned).
 * `out` is bit-identical with and without y.  Argument checks and error codes as lgcn_conv1d_gn.
 */
int64_t lgcn_conv_packed_f32_bytes(int cin, int cout, int ks);
int lgcn_conv_pack_weight_f32(const float *w, int cin, int cout, int ks, void *out, void *stream);
int lgcn_conv1d_gn_f32(const float *x, int64_t n_act, int lin, int cin, const void *wp, int cout, int ks, int stride,
                       const float *gamma, const float *beta, float eps, const float *res, int res_mode, int relu,
                       float *out, float *y /* NULL: inference */, void *stream);

/*
 * Optimizer step (reference utils.py:98-162: Optimizer.step = clip, then torch.optim's Adam / AdamW / SGD): the gradient
 * clamp and the update of many fp32 tensors, in place, in ONE launch.  Exact fp32, every operation rounded on its own
 * (no fused multiply-add), in the order of torch.optim's single-tensor path; one thread per element, no atomics, no
 * LDS, no scratch: bitwise repeatable.
 *
 * tensors : DEVICE array of n_tensors lgcn_opt_tensor_t.  p, g: parameter and gradient, n contiguous floats each.
 *           m: exp_avg (Adam / AdamW) or the momentum buffer (SGD; unused and may be NULL when momentum == 0).
 *           v: exp_avg_sq (NULL for SGD).  Any alignment of 4 bytes is accepted: a chunk whose four pointers are all
 *           16-byte aligned moves 16 bytes per access, any other chunk 4 bytes.  n == 0 is allowed.
 * chunks  : DEVICE array int32 [n_chunks][2] of (tensor id, first element); a chunk covers elements
 *           [first, min(first + lgcn_opt_chunk_elems(), n)) of its tensor, first % lgcn_opt_chunk_elems() == 0 (the
 *           chunk length is a multiple of 4).  The caller lists every chunk of every tensor it wants updated exactly
 *           once.  Workgroups of 256 threads grid-stride over the chunks (at most 2048 workgroups).  A row whose tensor
 *           id or first element lies outside its table, or whose tensor lacks a pointer the kind needs, is skipped.
 * One launch = one (parameter group, step count) segment: lr and the step count t are scalars of the launch.
 *
 * Per element, with the host's double hyper-parameters rounded to float once (w1 = 1 - beta1, w2 = 1 - beta2,
 * s = lr / bc1, r = sqrt(bc2), d = 1 - lr * wd), bc1 = 1 - beta1^t and bc2 = 1 - beta2^t computed by the caller in
 * double as torch.optim computes them:
 *   clip_on          : g = g < clip_low ? clip_low : g > clip_high ? clip_high : g, STORED to g (the reference clamps
 *                      p.grad in place); a NaN stays NaN, like clamp_.  Nothing else is written to g.
 *   LGCN_OPT_ADAM    : if wd: g' = g + wd * p (a temporary)      m = m + w1 * (g' - m)   [w1 >= 0.5: g' - (g' - m) * (1 - w1)]
 *                      v = v * beta2 + w2 * (g' * g')             p = p + (-s) * (m / (sqrt(v) / r + eps))
 *   LGCN_OPT_ADAMW   : if wd: p = p * d; then LGCN_OPT_ADAM with wd = 0.
 *   LGCN_OPT_SGD     : if wd: g' = g + wd * p.  momentum != 0: m = first_step ? g' : m * momentum + g'; g' = m.
 *                      p = p + (-lr) * g'.  (dampening 0, no Nesterov; momentum == 0: no buffer is read or written)
 * amsgrad and maximize are not implemented.  first_step is read by LGCN_OPT_SGD only (m is not read on it); beta1,
 * beta2, eps, bc1, bc2 by the Adam kinds only; momentum by LGCN_OPT_SGD only.
 *
 * Returns LGCN_EINVAL, launching nothing, for an unknown kind, n_chunks < 0, n_tensors < 0, a non-finite lr,
 * clip_on with clip_low > clip_high (or a NaN bound), an Adam kind with bc1 <= 0 or bc2 <= 0, and for n_chunks > 0
 * with a NULL table or n_tensors == 0.  n_chunks == 0 with valid scalars returns LGCN_OK without launching.
 */
enum { LGCN_OPT_ADAM = 0, LGCN_OPT_ADAMW = 1, LGCN_OPT_SGD = 2 };
typedef struct {
    float *p, *g, *m, *v;
    int64_t n;
} lgcn_opt_tensor_t;
int lgcn_opt_chunk_elems(void);
int lgcn_opt_step(const lgcn_opt_tensor_t *tensors, int n_tensors, const int32_t *chunks, int n_chunks, int kind,
                  double lr, double beta1, double beta2, double eps, double weight_decay, double momentum, int first_step,
                  double bc1, double bc2, int clip_on, float clip_low, float clip_high, void *stream);

/*
 * Goal decoder of the fork model (reference lanercnn.py:683-924): segmented greedy NMS, goal decoding and trajectory
 * refinement.  All three are exact fp32 with every operation rounded on its own (no fused multiply-add) in the
 * reference's order, asynchronous on `stream`, without workspace, floating-point atomics or host reads: bitwise repeatable.
 *
 * lgcn_nms_select -- nms_select (:687-708) for n_seg segments (RoIs) in one launch, one workgroup per segment.
 *   xys [n, 2], logits [n]; seg_off [n_seg + 1] int32, segment s = rows seg_off[s] .. seg_off[s + 1].
 *   The list of a segment:
 *     1. the survivors of greedy NMS in descending logit order: a node is dropped when
 *        sqrt(dx * dx + dy * dy) < threshold (strict; correctly rounded sqrt, compared as a distance, not as squares) for
 *        an already kept node;
 *     2. with fewer than min_len survivors, the highest-logit nodes not yet listed follow in descending logit order until
 *        the list has min_len entries or the segment is exhausted;
 *     3. the list is cut to max_keep entries (max_keep <= 0: no limit).
 *   Order of the logits, where torch.sort leaves it open: equal logits -- the lower index comes first; a NaN logit ranks
 *   above every number (as torch.sort(descending=True) ranks it), among NaNs the lower index comes first.
 *   idx [n] int32, segment-local: idx[seg_off[s] + j] = j-th entry of the list for j < count[s], -1 beyond; count [n_seg].
 *   A segment whose offsets do not lie in [0, n] in ascending order gets count 0 and its idx rows are not touched.
 *   LGCN_EINVAL: n < 0, n_seg < 0, min_len < 0, NaN threshold, NULL seg_off, or with work to do a NULL tensor;
 *   LGCN_ESHAPE: n > 2^28.  n_seg == 0: LGCN_OK without a launch.
 *
 * lgcn_goal_decode -- Decode.forward :802-865 for all n_agt interest agents in one launch, one workgroup per agent.
 *   pred [n, 5]: the goal head's rows of the interest RoIs, concatenated; pred_off [n_agt + 1] their spans (pred_off[0] = 0).
 *   anc_ctrs, anc_dirs [n_anc, 2]: the anchors of every RoI; anc_off [n_agt]: first anchor row of each interest RoI.
 *   pred_off_host / anc_off_host: the same two tables in HOST memory, read for the argument check only.
 *   agt_ctrs [n_agt, 2]; agt_dir_last [n_agt, 2] raw: d = dir / |dir|, and d = 0 where |dir| < 1e-6 (:845-848);
 *   agt_vel [n_agt]; k = num_mods (1..8).  Per agent, node i of its RoI:
 *     logit = pred[i, 0]    xy = anchor_ctr[i] + pred[i, 1:3]    theta = atan2(dir.y, dir.x) + atan(pred[i, 3] / pred[i, 4])
 *     top_idx = the lgcn_nms_select list of (xy, logit) with min_len = max_keep = k
 *   and per mode m with goal g = xy[top_idx[m]], p = (cos theta, sin theta), agent centre c (:710-723):
 *     a1 = (2 g.x d.x + 2 c.x d.x) / (2 + d.x - p.x)    a0 = g.x - c.x - a1    a2 = c.x       (b0, b1, b2: the same in y)
 *     L  = sum_j |P(j / 30) - P((j - 1) / 30)|, j = 1..30,  P(s) = (a0 s^2 + a1 s + a2, b0 s^2 + b1 s + b2)   (:851-855)
 *     acc = 2 (L - 3 vel) / 9    v_j = max(vel + acc * 0.1 j, 0)    s_samples[j - 1] = (v_0 + v_j) * 0.1 j / 2      (:856-861)
 *   (1.0 / 30 and 0.1 are rounded to fp32 before they multiply, as ATen rounds Python scalars.)
 *   Outputs: top_idx [n_agt, k] int32 RoI-local, goals [n_agt, k, 2], logits [n_agt, k], coef [n_agt, k, 6] =
 *   (a0, a1, a2, b0, b1, b2), s_samples [n_agt, k, 30] NOT normalised by its maximum (:900 adds to it as it is).
 *   LGCN_EINVAL: a negative size, k outside 1..8, NaN threshold, NULL host tables, pred_off_host[0] != 0, an interest
 *   RoI with fewer than k nodes (the reference fails there too, in torch.cat) or a span outside pred / the anchors,
 *   or with n_agt > 0 a NULL tensor.  n_agt == 0: LGCN_OK without a launch.
 *
 * lgcn_goal_refine -- Decode.forward :899-919, one wave per (agent, mode) row; n_rows = n_agt * k.
 *   s = s_samples[r] + traj_delta[r, :, 0];  s = s / max_t s (a NaN wins the maximum, as in torch.max);  exact zeros -> 1
 *   P = sample_trajectory(s) as above;  T = (2 a0 s + a1, 2 b0 s + b1) (sample_d1_trajectory);
 *   pred_trajs[r, t] = P + [[0, -1], [1, 0]] T * traj_delta[r, t, 1].
 *   s_samples [n_rows, 30], coef [n_rows, 6], traj_delta and pred_trajs [n_rows, 30, 2].
 *   LGCN_EINVAL: n_rows < 0 or with n_rows > 0 a NULL tensor.
 */
int lgcn_nms_select(const float *xys, const float *logits, const int32_t *seg_off, int64_t n, int n_seg,
                    float threshold, int min_len, int max_keep, int32_t *idx, int32_t *count, void *stream);
int lgcn_goal_decode(const float *pred, const int32_t *pred_off, const int32_t *pred_off_host, int64_t n,
                     const float *anc_ctrs, const float *anc_dirs, int64_t n_anc, const int32_t *anc_off,
                     const int32_t *anc_off_host, const float *agt_ctrs, const float *agt_dir_last,
                     const float *agt_vel, int n_agt, int k, float threshold, int32_t *top_idx, float *goals,
                     float *logits, float *coef, float *s_samples, void *stream);
int lgcn_goal_refine(const float *s_samples, const float *coef, const float *traj_delta, int64_t n_rows,
                     float *pred_trajs, void *stream);

/*
 * Training the goal decoder: the backward of lgcn_goal_refine and lgcn_goal_decode, one launch each.  Exact fp32 like
 * the forward (no fused multiply-add), asynchronous on `stream`, no workspace, no floating-point atomics, every sum in
 * a fixed order (bitwise repeatable), every output element written.  Nothing is saved by the forward besides top_idx:
 * both kernels recompute what they need with the forward's own operations, so the masks below are the forward's.
 * Not differentiated, as in the reference and in autograd of the stock ops: the selection top_idx; a speed that was
 * clamped (v_j <= 0, the reference's in-place v[v <= 0] = 0); a normalised sample that was exactly 0 and became 1.
 *
 * lgcn_goal_refine_bwd -- one wave per (agent, mode) row, n_rows = n_agt * k.  Inputs as lgcn_goal_refine plus
 *   d_pred_trajs [n_rows, 30, 2]; outputs d_s_samples [n_rows, 30], d_coef [n_rows, 6], d_traj_delta [n_rows, 30, 2].
 *   With s_t = s_samples[t] + delta[t, 0], mx = max_t s_t, u_t = s_t / mx, z_t = u_t (1 where u_t == 0), n_t = delta[t, 1],
 *   T = (2 a0 z + a1, 2 b0 z + b1) and g = d_pred_trajs[t]:
 *     d n_t  = g.y T.x - g.x T.y
 *     d z_t  = g.x T.x + g.y T.y + 2 n_t (g.y a0 - g.x b0)            d u_t = d z_t, 0 where u_t == 0
 *     d a0 = sum_t g.x z^2 + 2 g.y z n    d a1 = sum_t g.x z + g.y n    d a2 = sum_t g.x
 *     d b0 = sum_t g.y z^2 - 2 g.x z n    d b1 = sum_t g.y z - g.x n    d b2 = sum_t g.y
 *     d s_t  = d u_t / mx, and the first t with s_t == mx also receives -sum_t (d u_t u_t / mx)   (autograd's max + div)
 *     d_s_samples[t] = d_traj_delta[t, 0] = d s_t;   d_traj_delta[t, 1] = d n_t.
 *   LGCN_EINVAL: n_rows < 0 or with n_rows > 0 a NULL tensor; LGCN_ESHAPE: n_rows * 60 > 2^31 - 1.  n_rows == 0: LGCN_OK
 *   without a launch.
 *
 * lgcn_goal_decode_bwd -- one workgroup per interest agent.  Inputs: those of lgcn_goal_decode (threshold is not
 *   needed), the forward's top_idx [n_agt, k] and the upstream d_goals [n_agt, k, 2], d_logits [n_agt, k],
 *   d_coef [n_agt, k, 6], d_s_samples [n_agt, k, 30].  Output d_pred [n, 5]: the workgroup zero-fills its span, then one
 *   thread per mode fills row top_idx[m] (the entries of top_idx are distinct).  Per mode, in the notation of
 *   lgcn_goal_decode, with t_j = 0.1 j and s_j = j / 30:
 *     d acc  = sum_j d_s_samples[j - 1] (t_j / 2) t_j  over the j with v_j > 0         d L = 2 d acc / 9
 *     e_j = P(s_j) - P(s_(j-1)):   d a0 = d_coef[0] + sum_j d L (e_j.x / |e_j|) (s_j^2 - s_(j-1)^2)
 *                                  d a1 = d_coef[1] + sum_j d L (e_j.x / |e_j|) (s_j - s_(j-1))        (b0, b1: in y;
 *                                  a segment of length 0 passes nothing; a2 = c.x and b2 = c.y are inputs)
 *     a0 = g.x - c.x - a1, a1 = N / D, N = 2 g.x d.x + 2 c.x d.x, D = 2 + d.x - p.x:
 *       d g.x = d_goals.x + d a0 + (d a1 - d a0) 2 d.x / D            d p.x = (d a1 - d a0) a1 / D       (and in y)
 *     d theta = d p.y cos theta - d p.x sin theta;  theta includes atan(p3 / p4):
 *       d_pred[i] = (d_logits, d g.x, d g.y, d theta p4 / (p3^2 + p4^2), -d theta p3 / (p3^2 + p4^2)),  i = top_idx[m].
 *   LGCN_EINVAL: as lgcn_goal_decode, and pred_off_host[n_agt] != n (the spans must cover d_pred).  n_agt == 0: LGCN_OK
 *   without a launch.  An agent whose top_idx holds an index outside its RoI gets its zero rows only.
 */
int lgcn_goal_refine_bwd(const float *s_samples, const float *coef, const float *traj_delta, const float *d_pred_trajs,
                         int64_t n_rows, float *d_s_samples, float *d_coef, float *d_traj_delta, void *stream);
int lgcn_goal_decode_bwd(const float *pred, const int32_t *pred_off, const int32_t *pred_off_host, int64_t n,
                         const float *anc_ctrs, const float *anc_dirs, int64_t n_anc, const int32_t *anc_off,
                         const int32_t *anc_off_host, const float *agt_ctrs, const float *agt_dir_last,
                         const float *agt_vel, int n_agt, int k, const int32_t *top_idx, const float *d_goals,
                         const float *d_logits, const float *d_coef, const float *d_s_samples, float *d_pred, void *stream);

/*
 * RoiLoss of the fork model (reference lanercnn.py:1214-1301): one forward launch, one backward launch, the rules of
 * lgcn_pred_loss_fwd / _bwd (exact fp32, fixed-order sums, no atomics).  logits [n_agt, n_mod], goals [n_agt, n_mod, 2],
 * trajs [n_agt, n_mod, n_t, 2], gt [n_agt, n_t, 2], has [n_agt, n_t] bytes; n_mod in 1..8, n_t in 1..64.  Per agent
 * (none is dropped: without an observed step last = n_t - 1, the class term counts, the regressions do not):
 *   last    = argmax_t(has[t] + 0.1 t / n_t), first maximum, the fp32 values formed as in lgcn_pred_loss_fwd
 *   dist_j  = sqrt(|goals[j] - gt[last]|^2);  min_idx = first minimum
 *   cls    += sum_j (1 - y) x + max(-x, 0) + log(exp(-max(-x, 0)) + exp(-x - max(-x, 0))),  x = logits[j], y = (j == min_idx)
 *   goal   += SmoothL1(goals[min_idx] - gt[last]) (beta 1) if has[last]
 *   traj   += SmoothL1(trajs[min_idx, t] - gt[t]) over the t with has[t]
 * sums [3] = (cls, reg_coef * goal, reg_coef * traj); counts [3] int32 = (n_agt, #agents with has[last], #has);
 * sel [n_agt] int32 = min_idx | has[last] << 8; pred_goals [n_agt, 2] = goals[min_idx].
 * lgcn_roi_loss_bwd: given sel and the upstream gradients of the three sums (device scalars g_cls, g_goal, g_traj), writes
 * every element of dlogits (g_cls (sigmoid(x) - y)), dgoals and dtrajs (zero off the selected mode / unobserved steps).
 * LGCN_EINVAL: n_agt < 0, n_mod outside 1..8, n_t outside 1..64, or with n_agt > 0 a NULL tensor; LGCN_ESHAPE:
 * n_agt * n_mod * n_t * 2 > 2^31 - 1.  n_agt == 0: LGCN_OK without a launch (nothing is written: the sums of an empty
 * problem are the caller's zeros).
 */
int lgcn_roi_loss_fwd(const float *logits, const float *goals, const float *trajs, const float *gt, const unsigned char *has,
                      int64_t n_agt, int n_mod, int n_t, float reg_coef, float *sums, int32_t *counts, int32_t *sel,
                      float *pred_goals, void *stream);
int lgcn_roi_loss_bwd(const float *logits, const float *goals, const float *trajs, const float *gt, const unsigned char *has,
                      int64_t n_agt, int n_mod, int n_t, float reg_coef, const int32_t *sel, const float *g_cls,
                      const float *g_goal, const float *g_traj, float *dlogits, float *dgoals, float *dtrajs, void *stream);

/*
 * Lane-RoI extraction of the fork (reference data_lrcnn.py:620-844, generate_lane_roi) for a BATCH of scenes: the
 * per-agent lane search, the nodes of every RoI and the 14 induced relations, in four calls that share one struct.
 * Integer and exact-fp32 kernels (no FMA, correctly rounded sqrt): index arrays, feats, agent_feat and the distances
 * equal the reference's; lane lengths and step sums are added in numpy's order (pairwise_sum: 8 accumulators up to 128
 * elements, halves added recursively above, as numpy splits them), atan2f is the device's.
 * lgcn_roi_lane_length_host runs the kernels' lane-length routine on the host (feats [.,2] fp32, n node ids; NaN for a
 * negative n or a NULL array): the sum over sqrt(x * x + y * y) of the listed nodes, for comparison with numpy's bits.
 *
 * Inputs (device unless said): the scenes' arrays concatenated, indices LOCAL to their scene, int32.
 *   off_host / off_dev: one table of int32 offsets, the same on the host (validated) and on the device (read by kernels):
 *       node_off, lane_off, agent_off, slot_off, suc_off, pre_off: n_scenes + 1 entries each, from 0 to n_nodes, n_lanes,
 *       n_agents, n_slots, n_suc, n_pre; slot_off[s + 1] - slot_off[s] = agents(s) * lanes(s);
 *       then edge_off [14 * n_scenes + 1]: segment r * n_scenes + s holds relation r (pre 0..5, suc 0..5, left, right)
 *       of scene s in edge_u / edge_v, from 0 to n_edges.
 *   ctrs, feats, turn [n_nodes,2], control, intersect [n_nodes], lane_idcs [n_nodes];  a_ctrs [n_agents,2], a_feats,
 *   a_obs [n_agents,20,2] (steps and positions, 20 observed steps);  suc_pairs [n_suc,2], pre_pairs [n_pre,2] lane pairs.
 *   ws: lgcn_roi_ws_elems(n_nodes, n_lanes, n_edges, n_slots, n_agents) int32 (negative: LGCN_EINVAL for a negative size,
 *       LGCN_ESHAPE beyond 2^31 - 1 elements), kept from lgcn_roi_search to lgcn_roi_edge_fill.
 *
 * lgcn_roi_search (1 memset + 8 launches, 7 where one scan tile holds every row count): lanes -> nodes tables, the
 *   relations as CSR rows, then one workgroup per agent:
 *   speed (0: dropped), anchor node (closest node within pi/4 of the agent's heading, else pi/2, ties: smaller index; none:
 *   dropped), level-by-level lane search over suc_pairs (horizon v * 3 + horizon_buffer) and pre_pairs (v * 2 + ...), left /
 *   right closure, lane order (search order with every lane at its first occurrence when the closure adds none, else
 *   ascending).  agent_nodes [n_agents + 1]: the RoI's node count, 0 for a dropped agent (speed 0, no anchor, < 6 nodes,
 *   neither a pre[0] nor a suc[0] edge); the last word is a status: bit 0 = an index out of range was skipped (a node, lane
 *   or pair index of a relation, a lane pair or lane_idcs, whether or not an RoI would have reached it), bit 1 = a
 *   lane search hit lgcn_roi_max_levels() (a cycle of zero-length lanes).  agent_vel [n_agents].
 * lgcn_roi_nodes (1 launch): roi_agent [n_rois], roi_base [n_rois + 1] (node offset of every kept RoI, from the counts
 *   above) -> node_mask [n_out_nodes] int64, out_feats [n_out_nodes,8], agent_feat [n_rois,80], near [n_out_nodes]
 *   (distance to the agent < 5).
 * lgcn_roi_edge_count (1 launch): edge_cnt [n_rois * 15]: per RoI the edges of the 14 induced relations, then |a2m|.
 * lgcn_roi_edge_fill (1 launch): edge_base [n_rois * 15] (exclusive sums of edge_cnt: relations into out_u / out_v
 *   [n_out_edges] int64, a2m into a2m_v [n_out_a2m] int32) -> local (u, v), sorted by (u, v), each pair once.
 * No result depends on the arrival order of an atomic: the same inputs give the same bytes.
 *
 * Every call first checks, launching nothing on failure: NULL struct or required pointer, negative size, a table that does
 * not start at 0, decreases or ends elsewhere than its total (LGCN_EINVAL); misaligned pointers (LGCN_EALIGN, 16 bytes for
 * ws and the float2 arrays); a scene of more than lgcn_roi_max_lanes() = 4096 lanes, or a workspace beyond
 * 2^31 - 1 elements (LGCN_ESHAPE).  An empty batch (no agent / no RoI) returns LGCN_OK without a launch.
 */
typedef struct {
    int32_t n_scenes, n_agents, n_nodes, n_lanes, n_edges, n_slots, n_suc, n_pre;
    float horizon_buffer; int32_t n_rois;
    int32_t n_out_nodes, n_out_edges, n_out_a2m, pad_;
    const int32_t *off_host, *off_dev;
    const float *ctrs, *feats, *turn, *control, *intersect;
    const int32_t *lane_idcs;
    const float *a_ctrs, *a_feats, *a_obs;
    const int32_t *suc_pairs, *pre_pairs, *edge_u, *edge_v;
    int32_t *ws;
    int32_t *agent_nodes; float *agent_vel;                       /* lgcn_roi_search */
    const int32_t *roi_agent, *roi_base;                          /* lgcn_roi_nodes .. */
    int64_t *node_mask; float *out_feats, *agent_feat; int32_t *near;
    int32_t *edge_cnt;                                            /* lgcn_roi_edge_count */
    const int32_t *edge_base; int64_t *out_u, *out_v; int32_t *a2m_v;   /* lgcn_roi_edge_fill */
} lgcn_roi_t;
int lgcn_roi_max_lanes(void);
int lgcn_roi_max_levels(void);
float lgcn_roi_lane_length_host(const float *feats, const int32_t *nodes, int n);
int64_t lgcn_roi_ws_elems(int64_t n_nodes, int64_t n_lanes, int64_t n_edges, int64_t n_slots, int64_t n_agents);
int lgcn_roi_search(const lgcn_roi_t *p, void *stream);
int lgcn_roi_nodes(const lgcn_roi_t *p, void *stream);
int lgcn_roi_edge_count(const lgcn_roi_t *p, void *stream);
int lgcn_roi_edge_fill(const lgcn_roi_t *p, void *stream);
/*
 * lgcn_roi_edge_fill_graph (1 launch, in the place of lgcn_roi_edge_fill): the same rows, written as the indices of the
 * batch's MERGED block-diagonal graph, which the reference forms on the host from per-RoI arrays (data_lrcnn.py:690-844
 * builds them, lanercnn.py:122-231 -- subgraph_gather -- offsets and concatenates them): out_u / out_v = local index +
 * roi_base[r]; a2m_u [n_out_a2m] = r, a2m_v [n_out_a2m] = local node + roi_base[r], both int64 and arguments of this
 * entry (lgcn_roi_t is unchanged; its int32 a2m_v is not read).  edge_base may place the rows anywhere; given
 * RELATION-major (relation k of every RoI back to back in RoI order, then relation k + 1) every relation of the batch
 * graph is one run of out_u / out_v, in the order a concatenation over the RoIs gives.  Same kernel body (a template
 * flag), no further atomic or LDS.  Checks and codes: lgcn_roi_edge_fill's stage, a2m_v standing where its a2m_v stands,
 * a2m_u like it (NULL with n_out_a2m > 0: LGCN_EINVAL; not 8-byte aligned: LGCN_EALIGN).
 */
int lgcn_roi_edge_fill_graph(const lgcn_roi_t *p, int64_t *a2m_u, int64_t *a2m_v, void *stream);

/*
 * Device-resident scene store: the arrays of a flat store (lanegcn_amd/flatfile.py: S scenes, concatenated) stay in
 * device memory, and lgcn_store_gather cuts the FlatBatch and the actor-side extras of any B picked scenes out of them
 * in ONE launch.  Pure data movement: every output equals what FlatSceneFile.batch builds on the host, byte for byte.
 *
 * lgcn_store_t (device pointers, all read-only): node_ctrs, node_feats, turn [n_nodes,2], control, intersect [n_nodes],
 *   actor_ctrs [n_actors,2], actor_feats [n_actors,20,3], rot [n_scenes,2,2], orig [n_scenes,2], gt_preds
 *   [n_actors,30,2] fp32; has_preds [n_actors,30] bytes; edge_u, edge_v [n_edges] int32, scene-local.  gt_preds and
 *   has_preds: both or neither (NULL = the store has none; the batch's pointers for them are then not used).
 *
 * lgcn_store_batch_t: B = n_scenes picked scenes (repeats allowed), R = n_rel relations, G = 2 R B index segments;
 *   segment (r * 2 + w) * B + j holds relation r's u (w = 0) or v (w = 1) of the j-th picked scene.
 *   tab_host / tab_dev: the per-batch table, lgcn_store_table_elems(B, R) = 5 B + 2 G + 3 int64, the same on the host
 *   (validated) and on the device (read by the kernel):
 *       node_off [B + 1], actor_off [B + 1]   prefix sums of the OUTPUT rows, from 0 to n_nodes / n_actors
 *       node_src [B], actor_src [B]           first node / actor row of the picked scene in the store
 *       scene [B]                             the picked scene (rot, orig)
 *       seg_off [G + 1]                       prefix sums of idx_local, from 0 to n_elem
 *       seg_src [G]                           first element of the segment in edge_u / edge_v
 *   Outputs (device): node_ctrs, node_feats, turn [n_nodes,2], control, intersect [n_nodes], actor_ctrs [n_actors,2];
 *   node_off, actor_off [B + 1] int32; idx_local [n_elem], seg_off [G + 1], seg_base [G] int64 (seg_base = node_off of
 *   the segment's scene); actor_feats [n_actors,3,20] (transposed), rot [n_actors,2,2], orig [n_actors,2] (the scene's,
 *   per actor), gt_preds [n_actors,30,2], has_preds [n_actors,30].
 *
 * One launch over output elements; a thread finds its scene / segment by binary search in the table, so B and G are not
 * bounded by a wave or by LDS.  No atomics, no allocation, no host synchronisation.
 *
 * Checked before anything is launched: NULL struct, a negative size, a NULL pointer next to a non-zero size, only one
 * of gt_preds / has_preds, a prefix sum that does not start at 0, decreases or ends elsewhere than its total, a source
 * run or a scene outside the store (LGCN_EINVAL); n_nodes, n_elem, 60 n_actors, G or the table beyond 2^31 - 1
 * (LGCN_ESHAPE); pointers not aligned to 16 bytes ([.,2] arrays, rot, orig, the int64 arrays, tab_dev), 8 bytes (tab_host)
 * or 4 bytes (the rest but has_preds) (LGCN_EALIGN).  n_scenes == 0 with all totals 0 returns LGCN_OK without a launch.
 * lgcn_store_table_elems: LGCN_EINVAL for a negative argument, LGCN_ESHAPE beyond 2^31 - 1 elements.
 *
 * lgcn_store_gather_aug: the same launch (the same kernel body, its other instantiation) with the reference's training
 * rotation (data.py:45-63) applied on the way through.  aug_host / aug_dev: [B, 8] fp32, the same words on the host
 * (validated) and on the device (read by the kernel, 16-byte aligned); per picked scene Rm row-major, then rot'
 * row-major.  Every row (x, y) of node_ctrs, node_feats, actor_ctrs and of channels 0 / 1 of actor_feats becomes
 * (x Rm00 + y Rm10, x Rm01 + y Rm11): two fp32 products, each rounded, one fp32 add, no FMA.  rot [n_actors,2,2] is rot'
 * of the actor's pick instead of the store's; a scene picked twice is turned by the angle of each pick.  Everything
 * else is lgcn_store_gather's output, byte for byte.  Checked first: all that lgcn_store_gather checks, with the same
 * codes; then aug_host or aug_dev NULL, a non-finite entry of aug_host (LGCN_EINVAL), aug_dev not 16-byte aligned
 * (LGCN_EALIGN).  n_scenes == 0 returns as lgcn_store_gather does, without looking at the tables.
 *
 * lgcn_store_gather_pad: the same launch (the same kernel body, its third instantiation) for a batch padded to fixed
 * capacities.  The batch describes B + 1 = n_scenes scenes: B picked ones and, last, the FILLER scene, whose table
 * entries carry a negative source (node_src, actor_src, scene, and seg_src of its 2 R segments) and the lengths that
 * bring every total to its capacity: n_nodes, n_actors, n_elem are the capacities, the same for every batch, and so are
 * all kernel arguments and the grid -- only the contents of tab_dev change, which makes the launch replayable from a
 * captured graph.  The filler's rows are written without reading the store: node_ctrs (1e6, 1e6), every other node
 * array 0; its i-th actor has actor_ctrs (-1e6 - 256 i, -1e6), actor_feats, gt_preds, has_preds, orig 0 and rot the
 * identity; element e of a filler segment is e mod n_f (n_f = the filler's nodes): the scene-local self-loops of its
 * nodes.  Every element of every output array is written.  The real scenes' rows are lgcn_store_gather's.
 *   lgcn_store_pad_check(s, b, tab_host): host only, launches nothing, works without a GPU.  Everything
 *   lgcn_store_gather checks, with the same codes, on the table `tab_host` (b->tab_host is not read) for the B picked
 *   scenes; and: n_scenes < 2, n_nodes or n_actors 0 (the filler owns at least one node and one actor), a picked scene
 *   with a negative source or a last scene without one (LGCN_EINVAL); a filler with fewer than one node, one actor or
 *   zero elements in a segment -- the pick does not fit the capacities (LGCN_ESHAPE).
 *   lgcn_store_gather_pad(s, b, stream): checks the sizes, pointers and alignment as above and launches.  It reads
 *   neither b->tab_host nor any host table: call lgcn_store_pad_check on the words before they are uploaded to tab_dev.
 */
typedef struct {
    int64_t n_scenes, n_nodes, n_actors, n_edges;
    const float *node_ctrs, *node_feats, *turn, *control, *intersect;
    const float *actor_ctrs, *actor_feats, *rot, *orig, *gt_preds;
    const unsigned char *has_preds;
    const int32_t *edge_u, *edge_v;
} lgcn_store_t;
typedef struct {
    int32_t n_scenes, n_rel;
    int64_t n_nodes, n_actors, n_elem;
    const int64_t *tab_host, *tab_dev;
    float *node_ctrs, *node_feats, *turn, *control, *intersect, *actor_ctrs;
    int32_t *node_off, *actor_off;
    int64_t *idx_local, *seg_off, *seg_base;
    float *actor_feats, *rot, *orig, *gt_preds;
    unsigned char *has_preds;
} lgcn_store_batch_t;
int64_t lgcn_store_table_elems(int64_t n_scenes, int64_t n_rel);
int lgcn_store_gather(const lgcn_store_t *s, const lgcn_store_batch_t *b, void *stream);
int lgcn_store_gather_aug(const lgcn_store_t *s, const lgcn_store_batch_t *b, const float *aug_host, const float *aug_dev,
                          void *stream);
int lgcn_store_pad_check(const lgcn_store_t *s, const lgcn_store_batch_t *b, const int64_t *tab_host);
int lgcn_store_gather_pad(const lgcn_store_t *s, const lgcn_store_batch_t *b, void *stream);

/*
 * lgcn_store_pack: the write side of the store.  ONE launch packs G = n_seg index runs, each a contiguous piece of one
 * of K = n_src source arrays, back to back into dst [n_dst] int32, and (n_scenes > 0) cuts a batch's frame rows
 * [n_scenes,6] fp32 (orig, then rot row-major) into orig [n_scenes,2] and rot [n_scenes,2,2].  A source holds int16,
 * int32 or int64 elements; the conversion is numpy's astype(int32): int16 sign-extends, int64 keeps its low 32 bits.
 * It is how data_raw.build_store turns the builder's flat edge arrays (int64 scales, int16 left / right) into a store's
 * edge_u / edge_v, and how DeviceSceneStore.concat merges the edge arrays of P stores relation-major (P x 2R runs).
 *
 *   tab_host / tab_dev: lgcn_store_pack_table_elems(G, K) = 3 G + 1 + 3 K int64, the same on the host (validated) and
 *   on the device (read by the kernel; the source addresses live there, so K is not bounded by a kernel argument):
 *       seg_off [G + 1]   prefix sums of the destination words, from 0 to n_dst (empty runs allowed anywhere)
 *       seg_src [G]       the run's source, in [0, K)
 *       seg_at  [G]       first element of the run in its source
 *       src_ptr [K]       device address of the source (0 allowed for an empty source)
 *       src_kind [K]      bytes per element: 2, 4 or 8
 *       src_len [K]       elements of the source
 *   Words of dst beyond n_dst are not written.
 *
 * The grid lies over output words (then one thread per scene for the frame rows); a thread finds its run by binary
 * search in seg_off, so neither G nor a run's length is bounded by a wave, a workgroup or LDS.  No atomics, no
 * allocation, no host synchronisation.
 *
 * Checked before anything is launched: NULL struct, a negative size, n_seg == 0 next to a non-zero n_dst / n_scenes, a
 * NULL pointer next to a non-zero size, a kind other than 2 / 4 / 8, a negative source length, seg_off that does not
 * start at 0, decreases or ends elsewhere than n_dst, a source index outside [0, K), a run that begins or ends outside
 * its source (LGCN_EINVAL); n_dst, n_scenes, a source length or the table beyond 2^31 - 1 (LGCN_ESHAPE); tab_dev or rot
 * not 16-byte aligned, tab_host, frame or orig not 8-byte aligned, dst not 4-byte aligned, a source not aligned to its
 * element (LGCN_EALIGN).  n_seg == 0 returns LGCN_OK without a launch and without looking at the tables.
 * lgcn_store_pack_table_elems: LGCN_EINVAL for a negative argument, LGCN_ESHAPE beyond 2^31 - 1 elements.
 */
typedef struct {
    int64_t n_seg, n_src, n_dst, n_scenes;
    const int64_t *tab_host, *tab_dev;
    int32_t *dst;
    const float *frame;
    float *rot, *orig;
} lgcn_store_pack_t;
int64_t lgcn_store_pack_table_elems(int64_t n_seg, int64_t n_src);
int lgcn_store_pack(const lgcn_store_pack_t *p, void *stream);

/*
 * Resident lane-RoI store (lanegcn_amd/data_lrcnn.py: RoiStore): the lane RoIs of S scenes,
 * extracted once, stay in device memory, and lgcn_roi_store_gather cuts the merged RoI graph (data_lrcnn.RoiBatch) and
 * the per-RoI agent rows of any B picked scenes out of them in ONE launch.  Pure data movement: every output equals
 * what the extraction gives for the picked scenes alone, byte for byte.
 *
 * lgcn_roi_store_t (device pointers, all read-only; scene s owns one block of node rows and one block of RoIs):
 *   feats [n_nodes,8] fp32, node_mask [n_nodes] int32; agent_feat [n_rois,80], ctrs [n_rois,2], actor_feats, obs
 *   [n_rois,20,3], gt_preds [n_rois,30,2] fp32, has_preds [n_rois,30] bytes (gt_preds and has_preds: both or neither,
 *   NULL = the store has none); edge_u, edge_v [n_edges] int32, relation-major (pre 0..5, suc 0..5, left, right), the
 *   scenes back to back inside a relation; a2m_u, a2m_v [n_a2m] int32, scene after scene.  All indices are SCENE-LOCAL:
 *   the row within the block of the scene's RoI nodes, and for a2m_u the RoI's number within the scene.
 *
 * lgcn_roi_store_batch_t: B = n_scenes picked scenes (repeats allowed), G = 30 B index segments; segment q * B + j is
 *   run q of the j-th picked scene: q = 0..13 u of relation q, q = 14..27 v of relation q - 14, q = 28 a2m_u, q = 29 a2m_v.
 *   tab_host / tab_dev: the per-batch table, lgcn_roi_store_table_elems(B) = 4 B + 2 G + 3 int64, the same on the host
 *   (validated) and on the device (read by the kernel):
 *       node_off [B + 1], roi_off [B + 1]   prefix sums of the OUTPUT node rows / RoI rows, from 0 to n_nodes / n_rois
 *       node_src [B], roi_src [B]           first node row / first RoI of the picked scene in the store
 *       seg_off [G + 1]                     prefix sums of idx, from 0 to n_elem
 *       seg_src [G]                         first element of the segment in edge_u / edge_v / a2m_u / a2m_v
 *   Outputs (device): feats [n_nodes,8], node_mask [n_nodes] int64, agent_feat [n_rois,80], ctrs, actor_feats, obs,
 *   gt_preds, has_preds as in the store, and idx [n_elem] int64 = the resident int32 + the base of the picked scene:
 *   node_off[j], or roi_off[j] for a2m_u.  idx thus holds u (relation-major for the pick), v, a2m_u, a2m_v of the
 *   pick's merged graph back to back.
 *
 * One launch over output elements (16-byte pieces of the float rows, 2-byte pieces of has_preds, one index each); a
 * thread finds its scene / segment by binary search in the table, so B and G are not bounded by a wave, a workgroup or
 * LDS.  Every element of every output is written.  No atomics, no allocation, no host synchronisation.
 *
 * Checked before anything is launched: NULL struct, a negative size, a NULL pointer next to a non-zero size, only one
 * of gt_preds / has_preds, a prefix sum that does not start at 0, decreases or ends elsewhere than its total, a source
 * run outside the store (LGCN_EINVAL); 2 n_nodes, 81 n_rois, n_elem, G or the table beyond 2^31 - 1 (LGCN_ESHAPE);
 * pointers not aligned to 16 bytes (the float rows but ctrs, tab_dev), 8 bytes (ctrs, node_mask and idx of the batch,
 * tab_host), 4 bytes (the resident int32 arrays) or 2 bytes (has_preds) (LGCN_EALIGN).  n_scenes == 0 with all totals 0
 * returns LGCN_OK without a launch.
 * lgcn_roi_store_table_elems: LGCN_EINVAL for a negative argument, LGCN_ESHAPE beyond 2^31 - 1 elements.
 */
typedef struct {
    int64_t n_scenes, n_nodes, n_rois, n_edges, n_a2m;
    const float *feats;
    const int32_t *node_mask;
    const float *agent_feat;
    const int32_t *edge_u, *edge_v, *a2m_u, *a2m_v;
    const float *ctrs, *actor_feats, *obs, *gt_preds;
    const unsigned char *has_preds;
} lgcn_roi_store_t;
typedef struct {
    int64_t n_scenes, n_nodes, n_rois, n_elem;
    const int64_t *tab_host, *tab_dev;
    float *feats;
    int64_t *node_mask;
    float *agent_feat;
    int64_t *idx;
    float *ctrs, *actor_feats, *obs, *gt_preds;
    unsigned char *has_preds;
} lgcn_roi_store_batch_t;
int64_t lgcn_roi_store_table_elems(int64_t n_scenes);
int lgcn_roi_store_gather(const lgcn_roi_store_t *s, const lgcn_roi_store_batch_t *b, void *stream);

/*
 * Scene construction for a BATCH of raw scenes (lanegcn_amd/data_raw.py): tracks to actor arrays
 * (reference data.py:148-217, ArgoDataset.get_obj_feats) and map lanes to the scale-0 lane graph (data.py:220-361,
 * ArgoDataset.get_lane_graph up to :353; the dilated scales stay lgcn_bool_square*).
 *
 * Arithmetic, the same in both: per scene frame = (orig x, y, rot 00, 01, 10, 11) fp32, computed by the host; a point p
 * (float64) becomes d = p - (double)orig, x' = r00 * dx + r01 * dy, y' = r10 * dx + r11 * dy in float64, every product
 * and sum rounded on its own (no FMA).  Order comes from prefix scans (block scan + per-block sums: a scene may span any
 * number of workgroups); no float atomics: the same inputs give the same bytes.
 *
 * lgcn_scene_tracks (2 launches; data.py:162-201): off_host / off_dev = trk_off [n_scenes + 1] (tracks of every scene,
 *   from 0 to n_tracks; every scene holds at least its agent) then row_off [n_tracks + 1] (rows of every track, to
 *   n_rows), int32, the same on the host (validated) and on the device; xy [n_rows,2] float64 world positions, step
 *   [n_rows] int32 (>= 0; values of 50 and above are ignored), frame [n_scenes,6], pred_range = (x_min, x_max, y_min,
 *   y_max) compared in fp32.  Per track: steps 20..49 go to gt [.,30,2] (world, rounded to fp32) and has [.,30]; the
 *   track is kept if step 19 is present and its transformed, rounded position lies inside pred_range; its observed part
 *   is the maximal run of consecutive steps that ends at 19: obs [.,20,3] = (x', y', 1) rounded to fp32, ctrs [.,2] =
 *   obs[19], feats [.,20,3] = fp32 differences of obs with the run's first step zeroed.  Kept tracks are compacted in
 *   input order; the outputs hold n_tracks rows, of which the first head[n_scenes] are written.
 *   head [n_scenes + 2] int32, ZEROED by the caller: head[s] = first output row of scene s, head[n_scenes] = kept tracks,
 *   head[n_scenes + 1] = 0 or n_tracks - t for the first track t that lists a step below 50 twice (its output row, if
 *   any, is then unspecified).  ws: lgcn_scene_tracks_ws_elems(n_tracks) int32.
 *
 * Lane tables (lgcn_lane_table_t, one per city): topo_host / topo_dev = lgcn_scene_topo_elems(n_lanes, n_pred, n_succ)
 *   int32, the same on the host (validated by every call) and on the device: pt_off [L + 1], pred_off [L + 1], succ_off
 *   [L + 1], left [L], right [L], flags [L] (turn | control << 8 | intersect << 16; turn 1 = LEFT, 2 = RIGHT), pred
 *   [n_pred], succ [n_succ]; neighbours are table rows, -1 = not in the table; pts [n_pts,2] float64 on the device.
 *
 * lgcn_scene_lanes_rank (1 memset + 2 launches; data.py:228-241) and lgcn_scene_lanes_fill (2 launches; :243-334) share
 *   one struct.  tabs_host / tabs_dev [n_tables]: the same structs on the host and on the device.  off_host / off_dev:
 *   scene_tab [n_scenes] (table of every scene), cand_off [n_scenes + 1] (candidate lanes, to n_cand; at least one per
 *   scene), rank_off [n_scenes + 1] (prefix sums of the scenes' table sizes, to n_rank), and with explicit_ids != 0 cand
 *   [n_cand], the candidates as table rows in the caller's order, each row at most once per scene; with explicit_ids == 0
 *   the candidates of a scene are all rows of its table in table order.  pred_range is compared in float64.
 *   rank: a candidate is kept if the extent of its transformed centerline overlaps the rectangle; head [4 (n_scenes + 1)]
 *   = per scene, then in total, the exclusive sums of (kept lanes, their nodes, their pred entries, their succ entries).
 *   fill: n_nodes = head's node total; nodes in candidate order: ctrs, feats [n_nodes,2] (midpoint and difference of
 *   consecutive transformed points, formed in float64, rounded once), turn [n_nodes,2], control, intersect [n_nodes],
 *   lane_idcs [n_nodes] int64 (scene-local lane); pre_u / pre_v [cap_pre], suc_u / suc_v [cap_suc] int64: per lane its
 *   chain edges, then one edge per kept predecessor / successor in the table's list order (scene-local nodes); pre_pairs,
 *   suc_pairs, left_pairs, right_pairs [cap_*,2] int64 (scene-local lanes).  A neighbour is looked up in the per-scene
 *   rank array.  The caps are upper bounds from head (cap_pre >= nodes - lanes + pred entries, ...): a write beyond a cap
 *   is dropped, never made.  head2 [4 (n_scenes + 1)]: exclusive sums of the kept (pred, succ, left, right) neighbours;
 *   scene s owns pre edges [(node - lane + pred2)(s), ..(s + 1)) and so on.  ws: lgcn_scene_lanes_ws_elems(n_cand,
 *   n_rank) int32, kept from rank to fill.
 *
 * Checked before anything is launched: NULL struct or required pointer, negative size, NaN in pred_range, an offset table
 * that does not start at 0, decreases or ends elsewhere than its total, a scene without a track or a candidate, a lane of
 * fewer than 2 points, a neighbour row outside [-1, n_lanes), a table index or candidate outside its table, rank_off that
 * does not follow the table sizes (LGCN_EINVAL); misaligned pointers (LGCN_EALIGN: 16 bytes for ws, xy, pts, 8 for int64
 * arrays and tabs_dev, 4 for the rest); sizes beyond the 32-bit workspace, or a batch whose scenes' tables together hold more
 * than 2^31 - 1 points and neighbour entries, which the int32 scans could not count (LGCN_ESHAPE).  n_scenes == 0 with all totals 0
 * returns LGCN_OK without a launch.  The size helpers return LGCN_EINVAL / LGCN_ESHAPE as negative values.
 */
typedef struct {
    int32_t n_scenes, n_tracks, n_rows, pad_;
    float pred_range[4];
    const int32_t *off_host, *off_dev;
    const double *xy;
    const int32_t *step;
    const float *frame;
    int32_t *ws, *head;
    float *feats, *obs, *ctrs, *gt;
    unsigned char *has;
} lgcn_scene_tracks_t;
int64_t lgcn_scene_tracks_ws_elems(int64_t n_tracks);
int lgcn_scene_tracks(const lgcn_scene_tracks_t *p, void *stream);

typedef struct {
    int32_t n_lanes, n_pts, n_pred, n_succ;
    const int32_t *topo_host, *topo_dev;
    const double *pts;
} lgcn_lane_table_t;
typedef struct {
    int32_t n_scenes, n_tables, n_cand, n_rank, explicit_ids, pad_;
    double pred_range[4];
    const lgcn_lane_table_t *tabs_host, *tabs_dev;
    const int32_t *off_host, *off_dev;
    const float *frame;
    int32_t *ws, *head;                                            /* lgcn_scene_lanes_rank */
    int64_t n_nodes, cap_pre, cap_suc, cap_pre_pairs, cap_suc_pairs, cap_left_pairs, cap_right_pairs;
    int32_t *head2;                                                /* lgcn_scene_lanes_fill */
    float *ctrs, *feats, *turn, *control, *intersect;
    int64_t *lane_idcs, *pre_u, *pre_v, *suc_u, *suc_v, *pre_pairs, *suc_pairs, *left_pairs, *right_pairs;
} lgcn_scene_lanes_t;
int64_t lgcn_scene_topo_elems(int64_t n_lanes, int64_t n_pred, int64_t n_succ);
int64_t lgcn_scene_lanes_ws_elems(int64_t n_cand, int64_t n_rank);
int lgcn_scene_lanes_rank(const lgcn_scene_lanes_t *p, void *stream);
int lgcn_scene_lanes_fill(const lgcn_scene_lanes_t *p, void *stream);

/*
 * Graph construction for a BATCH of scenes (csrc/lgcn_graphbatch.hip): what lgcn_bool_square* and
 * lgcn_cross_edges do for one scene, from flat arrays plus per-scene offset tables, in a number of launches that does not
 * depend on the number of scenes.  Every output is an integer array and equals the per-scene entries' element for element
 * (the per-row bodies are shared, csrc/lgcn_graphops.hpp).  All offset tables are int32 [n_scenes + 1], start at 0, never
 * decrease and end at their total; off_host / off_dev hold the same tables, back to back, on the host (validated before
 * anything is launched) and on the device (read by the kernels).
 *
 * Dilation (reference data.py:520-534).  Tables: node_off, pre_off, suc_off.  pre_u / pre_v [n_pre], suc_u / suc_v [n_suc]:
 *   the scale-0 edges of every scene, int64, scene-local node indices (row u, column v); an edge with an end outside its
 *   scene's [0, n) is ignored.  ws: lgcn_dilate_batch_ws_elems(n_nodes, n_pre + n_suc) int32.
 *   lgcn_dilate_batch_csr   (1 launch + lgcn_csr_build): rowptr [lgcn_csr_rowptr_elems(2 n_nodes, 1)], col [n_pre + n_suc,
 *                            at least 1] = one CSR over the stacked rows (relation * n_nodes + scene base + node), columns
 *                            scene base + node.
 *   lgcn_dilate_batch_count (2 launches): out_rowptr [2 n_nodes + 1] = row pointer of A * A (exact, duplicate-free row
 *                            lengths; both relations and all scenes in one squaring); bounds [2][n_scenes + 1] = its value
 *                            where the scenes of the pre rows, then of the suc rows, begin and end.  Read bounds back:
 *                            bounds[1][n_scenes] = nnz, and bounds[r][s] - bounds[r][0] are the edge offsets of relation r.
 *   lgcn_dilate_batch_fill  (1 launch): out_col [nnz] (the next scale's col, with out_rowptr as its rowptr) and out_u /
 *                            out_v [nnz] int64, scene-local: rows ascending, columns ascending within a row, every edge
 *                            once; relation r owns [bounds[r][0], bounds[r][n_scenes]).  A row never writes beyond the
 *                            room out_rowptr gives it.
 *   The nnz of a scale must fit 31 bits.
 *
 * Left / right (reference preprocess_data.py:287-392, cross_angle = None).  Tables: node_off, lane_off, pre_off, suc_off,
 *   left_off, right_off (pairs per scene), then mask_off (sums of lanes^2), left_work_off and right_work_off (sums of
 *   side pairs * (pre pairs + suc pairs + 1)), which must be what the first six imply.  ctrs, feats [n_nodes,2] fp32,
 *   lane_idcs [n_nodes] int64 (scene-local lanes), the four pair lists [.,2] int64 (scene-local lanes); mat: 2 * mask_off[S]
 *   bytes (at most 0x7ffffff0, LGCN_ESHAPE beyond); ws: lgcn_cross_edges_batch_ws_elems(n_nodes) int32.
 *   lgcn_cross_edges_batch (1 memset + 4 launches, both sides together): out_u / out_v [2 n_nodes] int16 = the low 16 bits
 *   of the scene-local edge (u, partner of u), left side first, scenes in order, u ascending; counts [2][n_scenes + 1]:
 *   side d's edges of scene s are [counts[d][s], counts[d][s + 1]).  A scene whose side list is empty has no edge there.
 *
 * Refused before anything is launched: NULL struct or required pointer, negative size, NaN cross_dist, a bad offset table
 * (LGCN_EINVAL); pointers not aligned to 16 bytes (ws), 8 (int64 and float2 arrays), 4 (int32) or 2 (int16) (LGCN_EALIGN);
 * sizes beyond the 32-bit workspace or the mask limit (LGCN_ESHAPE).  n_scenes == 0 with all totals 0 returns LGCN_OK
 * without a launch.  The size helpers return LGCN_EINVAL / LGCN_ESHAPE as negative values.
 */
typedef struct {
    int32_t n_scenes, pad_;
    int64_t n_nodes, n_pre, n_suc;
    const int32_t *off_host, *off_dev;
    const int64_t *pre_u, *pre_v, *suc_u, *suc_v;                  /* lgcn_dilate_batch_csr */
    int32_t *ws, *rowptr, *col;
    int32_t *out_rowptr, *bounds;                                  /* lgcn_dilate_batch_count */
    int64_t nnz;                                                   /* lgcn_dilate_batch_fill */
    int32_t *out_col;
    int64_t *out_u, *out_v;
} lgcn_dilate_batch_t;
int64_t lgcn_dilate_batch_ws_elems(int64_t n_nodes, int64_t n_edges);
int lgcn_dilate_batch_csr(const lgcn_dilate_batch_t *p, void *stream);
int lgcn_dilate_batch_count(const lgcn_dilate_batch_t *p, void *stream);
int lgcn_dilate_batch_fill(const lgcn_dilate_batch_t *p, void *stream);

typedef struct {
    int32_t n_scenes;
    float cross_dist;
    int64_t n_nodes, n_lanes, n_pre, n_suc, n_left, n_right;
    const int32_t *off_host, *off_dev;
    const float *ctrs, *feats;
    const int64_t *lane_idcs, *pre_pairs, *suc_pairs, *left_pairs, *right_pairs;
    uint8_t *mat;
    int32_t *ws, *counts;
    int16_t *out_u, *out_v;
} lgcn_cross_batch_t;
int64_t lgcn_cross_edges_batch_ws_elems(int64_t n_nodes);
int lgcn_cross_edges_batch(const lgcn_cross_batch_t *p, void *stream);

/* ------------------------------------------------------------------ */
/* Forecasting metrics of a whole split (reference test.py:60-100)    */
/* ------------------------------------------------------------------ */

/*
 * lgcn_eval_scenes: one launch per batch, one wave per scene; no atomics, no host read.
 *   reg [A, M, T, 2] (world frame), cls [A, M], gt [A, T, 2] fp32; has [A, T] bytes; actor_off [B+1] int32
 *   (FlatBatch.actor_off); slot [B] int64: the row of each scene in the split-wide buffers, which the caller owns and
 *   zero-fills once: rec [n_slots, 32] fp32 and, both or neither, traj [n_slots, M, T, 2], score [n_slots, M].
 * Only the first actor row a = actor_off[b] of scene b is read (test.py:86).  rec[slot[b]]:
 *   [0] flag: 0 = not evaluated (no actor, or has[a, :horizon] not all set), 1 = evaluated, 2 = a non-finite value in
 *       reg[a, :, :horizon], cls[a] or gt[a, :horizon] (the has test comes first)
 *   [1] M, [2] horizon, [3] 0
 *   [4 + 3 (k - 1) + 0 / 1 / 2] = minFDE_k, minADE_k, p_k for k = 1..M, over the first k modes as they come:
 *       j* = first j < k of the smallest |reg[a, j, horizon - 1] - gt[a, horizon - 1]|; minADE_k = that mode's mean
 *       displacement over t < horizon (Argoverse: pick by FDE, report its ADE); p_k = softmax(cls[a, :k])[j*]
 *   every other float is 0; a record of flag 0 or 2 is 0 behind [0].  traj / score [slot[b]] = reg[a] / cls[a] for flag 1
 *   and 2.  A slot that no launch names is not touched.  The record depends on the scene's rows alone (not on B, the
 *   scene's place in the batch or the grid).
 *   err [1] int32: set to 1 when a slot[b] lies outside [0, n_slots); nothing is written for that scene.
 * lgcn_eval_reduce: one launch per summary, float64 in a fixed order (a strided pass, then a tree): bitwise repeatable.
 *   cnt [3] int64 = the slots with flag 0, 1, 2; out [8, 6] float64: row k - 1 = sums over the flag-1 records with
 *   M >= k of minADE_k, minFDE_k, [minFDE_k > miss_thr], (1 - p_k)^2 + minFDE_k, (1 - p_k)^2 + minADE_k,
 *   min(-log p_k, -log 0.05) + minADE_k (the numerators of Argoverse's minADE, minFDE, MR, brier-minFDE, brier-minADE,
 *   p-minADE).  err [1] int32: written 1 when two flag-1 records differ in [1] or [2], else 0.
 * Checked before any launch: LGCN_EINVAL (null pointer, negative size, M / T / horizon < 1, horizon > T, one of traj /
 * score alone), LGCN_ESHAPE (M > 8, T > 64, B or n_slots > 2^31 - 1), LGCN_EALIGN (any pointer but `has` not 16-byte
 * aligned).  B == 0 / n_slots == 0: LGCN_OK, nothing launched, nothing written.
 *
 * lgcn_eval_actors: the same record for EVERY actor row of the batch, partial futures included (the rule of PredLoss,
 * reference lanegcn.py:740-807): one launch per batch, one wave per actor row; no atomics, no host read.
 *   reg, cls, gt, has, actor_off as above; n_actors = A; slot_base [B] int64: the split-wide row of each scene's first
 *   actor (the split's actor_off[scene]); the tables hold one row per actor of the split.  Row a belongs to the scene b
 *   with actor_off[b] <= a < actor_off[b + 1] (scenes without actors are stepped over), i = a - actor_off[b], and its
 *   record goes to rec[slot_base[b] + i].  With O = {t < horizon : has[a, t]}, n_obs = |O|, t_last = max O:
 *   [0] flag: 0 = n_obs == 0; 2 = a non-finite value in reg[a, :, :horizon], cls[a] or gt[a, t] for t in O (an
 *       unobserved gt step is never looked at); 1 otherwise
 *   [1] M, [2] horizon (flag 1), [3] (float) i (every flag)
 *   [4 + 3 (k - 1) ...] as above with horizon - 1 -> t_last, the sum over t < horizon -> the sum over O, and the mean's
 *       divisor -> n_obs
 *   [28] horizon - n_obs (missing steps), [29] horizon - 1 - t_last (steps cut off the end) (flag 1)
 *   every other float is 0; a record of flag 0 or 2 is 0 in [1], [2], [4..31].  A fully observed first actor's record is,
 *   in all 32 floats, the one lgcn_eval_scenes writes for its scene.  traj / score rows: written for flag 1 and 2.
 *   err [1] int32: set to 1 when a row's slot lies outside [0, n_slots) or the row lies outside [actor_off[0],
 *   actor_off[B]); nothing is written for that row.
 *   Checks as lgcn_eval_scenes; LGCN_ESHAPE also for n_actors > 2^24 (a local index must be exact in fp32).
 *   n_actors == 0 / B == 0: LGCN_OK, nothing launched.
 * lgcn_eval_reduce_sel: lgcn_eval_reduce over the records a selection keeps -- the same thread-to-slot mapping, prefetch
 *   and tree, so out is bit for bit lgcn_eval_reduce's on a copy of the table whose excluded rows are zeroed.
 *   who: 0 all, 1 local index [3] == 0, 2 local index > 0 (any flag); max_missing: a flag-1 record counts only if
 *   [28] <= max_missing.  cnt [4] int64 = kept slots of flag 0, 1, 2, and the slots the selection excluded; err as in
 *   lgcn_eval_reduce, over the kept records.  LGCN_EINVAL also for who outside 0..2 or max_missing < 0.
 */
int lgcn_eval_scenes(const float *reg, const float *cls, const float *gt, const unsigned char *has,
                     const int32_t *actor_off, const int64_t *slot, int64_t n_scenes, int n_mod, int n_t, int horizon,
                     int64_t n_slots, float *rec, float *traj, float *score, int32_t *err, void *stream);
int lgcn_eval_reduce(const float *rec, int64_t n_slots, double miss_thr, double *out, int64_t *cnt, int32_t *err,
                     void *stream);
int lgcn_eval_actors(const float *reg, const float *cls, const float *gt, const unsigned char *has,
                     const int32_t *actor_off, const int64_t *slot_base, int64_t n_actors, int64_t n_scenes, int n_mod,
                     int n_t, int horizon, int64_t n_slots, float *rec, float *traj, float *score, int32_t *err,
                     void *stream);
int lgcn_eval_reduce_sel(const float *rec, int64_t n_slots, double miss_thr, int who, int max_missing, double *out,
                         int64_t *cnt, int32_t *err, void *stream);

/*
 * Drivable-area compliance (DAC), the map-side column of Argoverse's table, in the launch that writes the record.
 * A city's drivable area: a raster da_mat [h, w] (drivable iff == 1) and the first two rows m[6] = se2[0, 0..2],
 * se2[1, 0..2] of Argoverse's npyimage_to_city_se2, applied as stored to city coordinates.  A point (x, y) fp32 is INSIDE iff
 *   cx = rintf(x), cy = rintf(y) (round half to even, as np.round);
 *   u = cx m[0] + cy m[1] + m[2], v = cx m[3] + cy m[4] + m[5] in float64, unfused, left to right;
 *   iu = trunc(u), iv = trunc(v); 0 < iu < w and 0 < iv < h, both compared in float64 (row 0 and column 0 are left out as
 *   Argoverse leaves them out; a huge or NaN coordinate is outside, never an overflow); raster[off + iv w + iu] != 0.
 * Mode j of a row is COMPLIANT iff every step t < horizon of reg[a, j] is inside; has plays no part.
 *   lgcn_da_city_t: off = the first byte of the city's raster in `raster`, h, w, m.
 *   lgcn_drivable_t: raster = the cities' rasters back to back, raster_bytes bytes of (da_mat == 1), on the device; city
 *   [n_cities] on the device and city_host, the same table on the host (every check below reads the host copy; the
 *   kernel reads the device copy, the two must agree); scene_city [B] int32 on the device: the city id of each scene of
 *   the batch, -1 = no map.
 * lgcn_eval_scenes_da / lgcn_eval_actors_da: lgcn_eval_scenes / lgcn_eval_actors with two more floats in the record:
 *   [30] sum_j 2^j [mode j compliant], j < M <= 8 (exact)   [31] 1 when the scene's city has a raster
 *   both 0 for a record of flag 0 or 2 and for a scene of city id -1.  The other 30 floats, traj and score are bit for
 *   bit what the entries without `da` write (which leave [30], [31] at 0).  A city id outside [-1, n_cities) sets err [1]
 *   to 1; that row's record is written with [30] = [31] = 0.  No atomics, no second launch.
 *   Checked before any launch, after every check of the sibling: LGCN_EINVAL (da or one of its pointers null, n_cities < 1,
 *   raster_bytes < 0, a city with h or w < 1, off < 0 or a non-finite m in the host copy, a raster that does not lie
 *   inside raster_bytes), LGCN_ESHAPE (h or w > 2^31 - 1), LGCN_EALIGN (city or scene_city not 16-byte aligned).
 *   B == 0 / n_actors == 0: LGCN_OK, nothing launched, `da` not looked at.
 * lgcn_eval_dac_reduce: one launch per summary: dac [9] int64: dac[k - 1] = sum over the counted records with M >= k of
 *   popcount([30] & (2^k - 1)), dac[8] = n_dac, the counted records: flag 1, [31] == 1, kept by the selection (who,
 *   max_missing) of lgcn_eval_reduce_sel (who = 0 and max_missing >= horizon keep all).  DAC_k of the split =
 *   dac[k - 1] / (k n_dac).  Integer sums: exact, whatever the order.  LGCN_EINVAL (null pointer, n_slots < 0, who outside
 *   0..2, max_missing < 0), LGCN_ESHAPE (n_slots > 2^31 - 1), LGCN_EALIGN; n_slots == 0: LGCN_OK, nothing launched.
 */
typedef struct {
    int64_t off, h, w;
    double m[6];
} lgcn_da_city_t;
typedef struct {
    const uint8_t *raster;
    int64_t raster_bytes;
    const lgcn_da_city_t *city, *city_host;
    int32_t n_cities;
    const int32_t *scene_city;
} lgcn_drivable_t;
int lgcn_eval_scenes_da(const float *reg, const float *cls, const float *gt, const unsigned char *has,
                        const int32_t *actor_off, const int64_t *slot, int64_t n_scenes, int n_mod, int n_t, int horizon,
                        int64_t n_slots, float *rec, float *traj, float *score, int32_t *err, const lgcn_drivable_t *da,
                        void *stream);
int lgcn_eval_actors_da(const float *reg, const float *cls, const float *gt, const unsigned char *has,
                        const int32_t *actor_off, const int64_t *slot_base, int64_t n_actors, int64_t n_scenes, int n_mod,
                        int n_t, int horizon, int64_t n_slots, float *rec, float *traj, float *score, int32_t *err,
                        const lgcn_drivable_t *da, void *stream);
int lgcn_eval_dac_reduce(const float *rec, int64_t n_slots, int who, int max_missing, int64_t *dac, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LGCN_H */
