/*
 * genie_hip.h — C ABI of libgenie_hip.so: MI355X (gfx950) kernels for GENIE's station <-> source-grid
 * message-passing hot path.
 *
 * The reference (imcbrearty/GENIE) is pure Python: it has NO plugin / FFI interface. The boundary this
 * library replaces is the body of three `torch.nn.Module.forward` methods and the third-party kernels they
 * call (PyG `MessagePassing.propagate`, `torch_scatter.scatter`):
 *
 *   DataAggregation.forward            /root/reference/Code/module.py:85-98
 *   BipartiteGraphOperator.forward     /root/reference/Code/module.py:224-229
 *   SpatialAggregation.forward/message /root/reference/Code/module.py:243-249
 *
 * as called from GCN_Detection_Network_extended.forward / forward_fixed / forward_fixed_source
 * (module.py:916-920, :973-977, :1010-1014). Each entry point below cites the lines it replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to contiguous memory (e.g. torch `tensor.data_ptr()`), fp32 or int32;
 *  - `stream` is a `hipStream_t` passed as `void*` (NULL = default stream); calls enqueue work and return,
 *    they never synchronise and never allocate in the hot path;
 *  - the caller owns every input / output / workspace buffer; the library owns only what `genie_ctx_create`
 *    copies (base graphs, processing order) and its weight mirror; `genie_ctx_destroy` frees them;
 *  - return value 0 = ok, negative = error; `genie_last_error()` gives the message (thread-local);
 *  - product-graph node id p = g * n_sta + s (process_utils.py:720-722). Source nodes [0, n_grid) are OWNED by
 *    this context; source nodes [n_grid, n_grid_ext) are HALO rows (owned by another GPU when the grid is
 *    sharded over source nodes) that only appear as neighbours in `src_col`;
 *  - arithmetic: fp32 in, fp32 out, fp32 accumulation everywhere. On the reference's kNN graphs (8 station / 15 source
 *    neighbours) the P-sized stages multiply on the 16-bit matrix pipe with every fp32 operand as two fp16 pieces (x within
 *    one fp32 ulp, three partial products per product): fp32-class results, which need every hidden state of DataAggregation
 *    below 65504 in magnitude. The library checks that itself: at every weight commit it bounds those hidden states rigorously
 *    from the weights (inputs Slice, Mask in [-1, 1], as the reference produces them) and runs the fp32-MFMA kernels instead
 *    whenever the bound exceeds the fp16 range (genie_set_stage_precision / genie_stage_precision). edge_attr must stay
 *    below 65504 in magnitude (it is (grid - station) / scale_x_extend, process_continuous_days.py:630: O(1)).
 */
#ifndef GENIE_HIP_H
#define GENIE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct genie_ctx genie_ctx;

#define GENIE_OK 0
#define GENIE_ERR_ARG (-1)
#define GENIE_ERR_HIP (-2)
#define GENIE_ERR_STATE (-3)

/* Library / ABI version (major*100 + minor). */
int genie_version(void);
/* Message of the last error raised on this thread ("" if none). */
const char* genie_last_error(void);

/*
 * Create a context for one (stations x source-grid) product graph.
 * Replaces the graph objects cached by `set_adjacencies` (module.py:941-961); the inputs are the BASE kNN
 * graphs of process_utils.py:718-719 in CSR form (in-edges grouped by target), not the [2,E] product lists
 * of :720-721 — the Cartesian structure makes those implicit.
 *   sta_rowptr[n_sta+1], sta_col[sta_rowptr[n_sta]]   : station j -> station i edges, col = neighbour j
 *   src_rowptr[n_grid+1], src_col[src_rowptr[n_grid]] : source-node edges for OWNED nodes; col in [0,n_grid_ext)
 *   grid_order[n_grid]   : processing order of owned source nodes (a space-filling-curve order keeps the
 *                          neighbour rows of concurrently processed nodes in one XCD's L2); NULL = identity
 * All index arrays are int32 DEVICE pointers and are copied.
 */
int genie_ctx_create(genie_ctx** out, int n_sta, int n_grid, int n_grid_ext,
                     const int32_t* sta_rowptr, const int32_t* sta_col,
                     const int32_t* src_rowptr, const int32_t* src_col,
                     const int32_t* grid_order, float scale_rel);
/* Irregular product graph (`use_subgraph: True`, config.yaml:86; built by extract_inputs_adjacencies_subgraph,
 * process_utils.py:744-849): the product nodes are an explicit list of n_prod (station, source) pairs GROUPED BY SOURCE NODE
 * (process_utils.py:790-794), so `seg_rowptr[g] .. seg_rowptr[g+1]` is the row range of source node g (seg_rowptr[n_grid] =
 * n_prod), and both DataAggregation edge sets are CSR lists over product-node ids: p_sta_* = in-edges of A_in_sta (same
 * source node, neighbouring stations), p_src_* = in-edges of A_in_src, in stable edge order. src_rowptr / src_col = the base
 * source graph A_src (SpatialAggregation). Every [P, .] argument of the stage calls then has n_prod rows. The kernels that rely on
 * p = g * n_sta + s are not used (product-level CSR forms instead, inference and training); genie_nbr_mean is unavailable on such a
 * context, genie_embed_window* needs genie_set_subgraph_stations first; genie_set_edge_features / genie_set_absolute_pos take
 * positions per product node there ([n_prod, 3]). */
int genie_ctx_create_subgraph(genie_ctx** out, int n_sta, int n_grid, int64_t n_prod,
                              const int32_t* p_sta_rowptr, const int32_t* p_sta_col,
                              const int32_t* p_src_rowptr, const int32_t* p_src_col, const int32_t* seg_rowptr,
                              const int32_t* src_rowptr, const int32_t* src_col, const int32_t* grid_order, float scale_rel);
/* One rank's part of an irregular product graph sharded over source nodes: an irregular context over an EXTENDED row list. The n_own
 * owned source nodes are numbered in the order the rank processes them and their product rows come first, node after node
 * (seg_rowptr [n_own + 1], seg_rowptr[n_own] = n_prod_own); rows [n_prod_own, n_prod_ext) are HALO rows: product nodes of source nodes
 * owned elsewhere. p_sta_* / p_src_* are the product-level CSRs of the n_prod_own owned rows with columns in this local numbering:
 * station neighbours are owned rows, source neighbours owned or halo rows, in the edge order of the unsharded lists (every column is
 * checked against those bounds here; GENIE_ERR_ARG). Slice / Mask (and genie_set_subgraph_stations, genie_embed_window*) have
 * n_prod_ext rows, every other [P, .] argument and the c / wu rows n_prod_own; the wv rows (genie_ws_v_ptr) have n_prod_ext, the halo
 * part filled by the caller between the two stages. Because a range of source nodes is a range of rows, genie_da_stage1_range and
 * genie_da_stage2_partials_range are served on such a context (on genie_ctx_create_subgraph they are not), with genie_da_stage1,
 * genie_da_stage2_partials and genie_bipartite_readout; every kernel cuts its tiles from the first row of the range or of the source
 * node, so each row's and each node's result is the unsharded context's, bit for bit. Inference only and the default model
 * definition: the training calls, genie_assoc_fwd*, genie_set_edge_features and genie_set_absolute_pos return GENIE_ERR_STATE, and
 * no base source graph is kept (nothing G-sized runs on it). */
int genie_ctx_create_subgraph_ext(genie_ctx** out, int n_sta, int n_own, int64_t n_prod_own, int64_t n_prod_ext,
                                  const int32_t* p_sta_rowptr, const int32_t* p_sta_col,
                                  const int32_t* p_src_rowptr, const int32_t* p_src_col, const int32_t* seg_rowptr, float scale_rel);
/* Station index of every product node of an irregular product graph (device pointer, n_prod int32 = row 0 of the reference's
 * A_src_in_sta, process_utils.py:790-794; copied): what the device embedding reads where a Cartesian graph has p % n_sta. `trv` of
 * genie_embed_window* is then [n_prod, 2], the travel times of the listed (station, source) pairs
 * (`trv_times[src, ind_use[sta], :]`, process_utils.py:605). */
int genie_set_subgraph_stations(genie_ctx* ctx, const int32_t* sta_of_prod, void* stream);
int genie_ctx_destroy(genie_ctx* ctx);
/* Accounting of the library's device-memory pool on `device` (every buffer a context owns comes from it; freed blocks are cached and
 * handed out again): blocks / bytes handed out and not returned (`live`), bytes sitting in the free lists (`cached`). Any output
 * pointer may be NULL. Host-only and read-only: no driver call, no synchronisation. After genie_ctx_destroy the `live` figures are
 * back where they were before the matching create (the per-device model tables of the first context stay live). */
int genie_pool_stats(int device, int64_t* live_blocks, int64_t* live_bytes, int64_t* cached_bytes);
/* Optional station processing order: `order` (HOST pointer, n_sta int32, a permutation; typically the stations sorted along a
 * space-filling curve) = the caller's station id of the i-th station processed. A tile of the P-sized kernels is 16 consecutive
 * stations of one source node, and a station's neighbours are its nearest stations: with spatially sorted stations the rows a
 * tile gathers are shared between its lanes and adjacent in memory (config 2: stage 2 -6 %, config 4 with 2000 stations: whole
 * path -10 %). Purely internal: every input and output keeps the caller's station order (the split rows, c / wu / wv live in
 * processing order inside the workspace; genie_ws_export un-permutes). Honoured by the f16x2 stage 1 + pipelined stage 2
 * pair on Cartesian product graphs, ignored otherwise; NULL = off. All ranks of a sharded run must pass the same order. */
int genie_set_station_order(genie_ctx* ctx, const int32_t* order);
/* `use_phase_types: False` (config.yaml:91): genie_embed_window* then writes zeros into the phase-informed columns 2, 3 of Slice /
 * Mask (process_continuous_days.py:783-786); the caller passes every pick with phase 0 (:562-563) and zeroes `phase_label` for the
 * association heads (module.py:632-633, :706-707). Default: phase types in use. */
int genie_set_phase_types(genie_ctx* ctx, int use_phase_types);
/* `use_sign_input: True` (config.yaml:93; process_utils.py:610-614, the `use_sign_input` argument of extract_input_from_data): the
 * device embedding (genie_embed_window*) multiplies each of the four features of a product node by the sign of the NEGATIVE forward
 * difference of the series it is read from, at the index it is read at (+1 on the falling side of a pick's kernel, -1 on the rising
 * side, 0 on a flat stretch); Mask = |Slice| > 0.01 as before. Default off. */
int genie_set_sign_input(genie_ctx* ctx, int use_sign_input);
/* Work map of the row-layout stage 2 (k_stage2_ord: the association pass, the training forward of other graph shapes): 1 = blocks of 4
 * adjacent source nodes per workgroup, one node per wave (the default from 1024 stations up: the gathers leave L2 there and locality
 * pays), 0 = interleaved items, -1 = the default for the context's station count. Results do not depend on it (tests). The library reads
 * no environment variable; this is the one scheduling choice a caller can make. */
int genie_set_stage2_workmap(genie_ctx* ctx, int blocks_of_four);
/* Station tail tiles of the f16x2 stage 1 (k_stage1_h2) on a Cartesian graph: with n_sta mod 16 in 1 .. 8 the half-empty last station
 * tiles of two adjacent source nodes share one 16-lane row (on != 0, the default); 0 = every node keeps its own padded tail tile, the
 * earlier item table, kept for A/B runs and the byte-equality tests. Results do not depend on it, to the bit (tests). Other station
 * counts and other kernels have nothing to pack and ignore it. */
int genie_set_tail_packing(genie_ctx* ctx, int on);
/* Arithmetic of the G-sized tail of inference calls (Bipartite read-out, SpatialAggregation x3, SpatialDirect + TemporalAttention
 * on the grid): fp64_chains != 0 (default) = every Linear as a chain of fp64 MFMAs on the fp32 inputs and weights, fp64 PReLUs
 * and sums, one rounding to fp32 per kernel; 0 = fp32 MFMA chains (the arithmetic of the training forward, and the A/B form).
 * The fp32 chains are where almost all of the distance between (y, x) and the reference's fp64 run is made. */
int genie_set_tail_precision(genie_ctx* ctx, int fp64_chains);
/* Arithmetic of the P-sized stages on the reference's kNN graphs. mode 0 (default) = automatic: two-piece fp16 operands on the
 * 16-bit matrix pipe (k_stage1_h2 / k_stage2_h2u) while the fp16 range guard of the committed weights holds, the fp32-MFMA kernels
 * otherwise; 1 = two-piece fp16 operands regardless of the guard (A/B runs; hidden states above 65504 become non-finite);
 * 2 = fp32 MFMA always. No environment variable takes part. */
int genie_set_stage_precision(genie_ctx* ctx, int mode);
/* What runs for the weights committed so far (commits pending ones): *mode as set, *f16x2_active 1 / 0, and the two numbers
 * the range guard compares with 60000: the largest rigorous bound of a hidden state that is split into fp16 pieces, and the
 * largest weight magnitude in the form that is rounded to fp16. Any out pointer may be NULL. Synchronises `stream` when weights
 * were pending (the guard's 16-byte read-back). */
int genie_stage_precision(genie_ctx* ctx, int* mode, int* f16x2_active, float* act_bound, float* weight_bound, void* stream);
/* Input range of the f16x2 kernels (round 5). The range guard above holds for inputs in [-1, 1] (process_utils.py:262-275, :610-629: the
 * only inputs the reference's pipeline produces) and, its bound being linear in the input magnitude, up to |input| <= *limit = 60000 /
 * act_bound. The split pass of every f16x2 stage-1 call checks the rows it reads and records the largest magnitude BEYOND that limit in a
 * word of host-mapped memory; this call returns it in *max_seen (0 = every input so far was inside the limit) WITHOUT synchronising: it
 * reflects the split passes that have completed. reset != 0 = ONE atomic fetch-and-clear: the value returned is exactly the value cleared
 * (kernels still in flight may be writing the word: a read followed by a separate store could drop what they wrote in between). Nobody
 * reads the word once the context is destroyed: check after the LAST call on a context too (the Python host does when it replaces a
 * context, at the read-backs it makes anyway, and warns from the destructor). A caller that sees a non-zero value must discard the
 * results of the calls issued since its last check and switch to genie_set_stage_precision(ctx, 2) (the Python host does both and
 * raises). Never set by the fp32 kernels, by the device embedding's split rows (values in [-1, 1] by construction) or in mode 2. */
int genie_input_range(genie_ctx* ctx, float* max_seen, float* limit, int reset);
/* Index errors found on the device since the last reset, read from host-mapped memory without synchronising (like genie_input_range):
 * bit 0 = a pick of a genie_lslc_fwd call indexed outside the time-pointer table (tpick outside dt_partition, or ipick outside the
 * stations of A_edges; the kernel clamps the index, the reference's indexing at Code/module.py:635-640 fails with a device-side
 * assertion reported at its next synchronisation). reset != 0 = atomic fetch-and-clear (see genie_input_range). The Python host raises
 * IndexError at its next call on the context, where it has just waited for the device anyway, and when it replaces the context. */
int genie_index_flags(genie_ctx* ctx, unsigned* flags, int reset);
/* Range check of a caller's index list on the device, no host round trip: sets `bit` (2, 4, ...; bit 0 belongs to genie_lslc_fwd) in the
 * word genie_index_flags returns when some idx[i] lies outside [lo, hi). The Python host uses bit 1 (value 2) for the station indices
 * `ipick` of the Arrivals head (Code/module.py:703-713 indexes `trv_out[:, ipick]` with them), which it clamps for its own use. */
int genie_index_check(genie_ctx* ctx, const int64_t* idx, int64_t n, int64_t lo, int64_t hi, unsigned bit, void* stream);
/* With a station processing order: registers the caller's STATIC edge_attr [P, 3] (A_src_in_edges.x, process_utils.py:722: a
 * function of the geometry only); the library keeps it in the form stage 2 consumes (two-piece fp16 operand fragments in
 * processing order, 32 B per product node) and uses that in every stage-2 call that is passed this same pointer; any other
 * edge_attr is converted per call. Call again if the contents change; NULL unregisters. No-op without a station order. */
int genie_set_static_edge_attr(genie_ctx* ctx, const float* edge_attr, void* stream);
/* Every buffer of the workspace that carries data from one call to the next (stage 1 -> stage 2: c, wu, wv; stage 2 ->
 * tail: Bipartite partials; SpatialAggregation / read-out scratch) exists several times; `slot` (0..15) selects the copy
 * used by the calls issued next (33 copies of the G-sized buffers: two batches of 16 windows in flight and one for single-stream calls; the P-sized rows have 4, indexed slot % 4). With several HIP streams a caller can run stage 1 of window i+1 (MFMA-bound), stage 2 of window
 * i (HBM-bound) and the G-sized tail of window i-1 (latency-bound) concurrently: all calls of one window use the same
 * slot, consecutive windows rotate through the slots, and the caller orders "stage 1 of window i+2 after stage 2 of window i" etc. with
 * events. Default slot 0. */
int genie_set_slot(genie_ctx* ctx, int slot);
/* The G-sized tail of `nwin` windows (whose stage-2 partials sit in slots slot0 .. slot0+nwin-1) in one set of launches:
 * Bipartite read-out, SpatialAggregation x3 -> x_spatial_out [nwin, G, 30], y_out [nwin, G, n_t] (genie_readout_grid) and,
 * if x_out != NULL, x_out [nwin, n_query, n_t] (genie_readout_query). Bit-identical to the per-window calls; replaces
 * nwin x (genie_bipartite_readout + genie_spatial_agg3_fwd + genie_readout_grid + genie_readout_query) in the apply
 * loop (process_continuous_days.py:761-810), whose windows are independent. */
int genie_tail_batched(genie_ctx* ctx, int slot0, int nwin, const float* pos, const float* x_query, const int32_t* knn,
                       int n_query, int k, const float* t_query, int n_t, float* x_spatial_out, float* y_out, float* x_out,
                       void* ws, void* stream);
/* genie_tail_batched with a query set per window (the refine pass: every candidate source has its own query cloud): x_query [n_sets,
 * n_query, 3], knn [n_sets, n_query, 10] and qset [nwin] int32 on the device; window w is read out at the queries of set qset[w], i.e. its
 * query nl reads row qset[w] * n_query + nl of x_query and knn, and x_out [nwin, n_query, n_t] row w is genie_tail_batched's for that
 * set. Everything else (slots, x_spatial_out, y_out, streams) as genie_tail_batched; bit-identical to the per-window calls. CONTRACT:
 * every qset[w] lies in [0, n_sets). The library does not read the table on the host and the kernel does not check it: a caller that
 * knows the values checks them (the Python binding does, before any launch). Refused with GENIE_ERR_ARG: a null qset, n_sets < 1, a
 * null x_out, n_sets * n_query or nwin * n_query above INT_MAX, and what genie_tail_batched refuses (a sharded context:
 * GENIE_ERR_STATE). */
int genie_tail_batched_q(genie_ctx* ctx, int slot0, int nwin, const float* pos, int n_sets, const int32_t* qset, const float* x_query,
                         const int32_t* knn, int n_query, int k, const float* t_query, int n_t, float* x_spatial_out, float* y_out,
                         float* x_out, void* ws, void* stream);
/* Temporal scale of TemporalAttention: `scale_t = 3 * kernel_sig_t` (module.py:40); default 9.0. */
int genie_set_scale_t(genie_ctx* ctx, float scale_t);
/* `use_absolute_pos: True` (config.yaml:92; module.py:916, :971, :1007): every product node's input gets its station position and
 * its source position, each divided by 3 * scale_rel, appended (in_channels 4 -> 10). Positions are [n_sta,3] / [n_grid_ext,3]
 * fp32 device pointers; the 6 extra columns of init_trns.weight go to the registry entry "DataAggregation.init_trns.weight_abs"
 * ([30,6] = weight[:, 4:10]) and "DataAggregation.init_trns.weight" keeps the [30,8] layout (weight[:, [0:4, 10:14]]). The
 * neighbours' hidden states are recomputed with their own positions (one more K-step per neighbour in the f16x2 stage-1 kernel;
 * two k-steps in the generic fp32-MFMA kernel that serves ragged graphs). Null = off. */
int genie_set_absolute_pos(genie_ctx* ctx, const float* pos_sta, const float* pos_src, void* stream);
/* DataAggregationEdges variant (`use_updated_model_definition: True`, config.yaml:95; module.py:102-174): every message is
 * [x_j || phi(pos_j - pos_i) || phi(|pos_j - pos_i|)], phi(d) = sign(d) exp(-d^2 / (2 scale_rel^2)) (forward :1059-1072,
 * set_adjacencies :1102-1111). On the product graph the mean of those 4 edge features is a static vector per station
 * (station graph) / per source node (source graph); the library computes them from the positions ([n_sta,3] and
 * [n_grid_ext,3] device pointers, fp32) and applies the 4 edge-feature columns of l1_t?_2 / l2_t?_2 (registry entries
 * "DataAggregation.l?_t?_2.weight_pos", [out,4]) as per-node additive terms. The other columns keep the DataAggregation
 * layout: the caller passes `l1_t?_2.weight[:, [0:60, 64:68]]` and `l2_t?_2.weight[:, [0:90, 94:98]]` under the usual names.
 * Null positions switch back to plain DataAggregation. On an irregular product graph (genie_ctx_create_subgraph) the mean runs over
 * the PRESENT neighbours of a product node: both arguments are then [n_prod, 3] (the station's / the source node's position of every
 * product node) and the additive terms are per product node. */
int genie_set_edge_features(genie_ctx* ctx, const float* pos_sta, const float* pos_src, void* stream);

/*
 * Weight mirror. Parameter names are the reference's state_dict keys (e.g. "DataAggregation.l1_t1_2.weight",
 * layout [out, in] row-major exactly as nn.Linear stores it; PReLU slopes are 1-element tensors).
 * Enumerate with genie_weights_count/name/numel; copy with genie_weights_set (async D2D on `stream`).
 * The MFMA-fragment repack happens lazily on the next forward call (or explicitly with genie_weights_commit).
 */
int genie_weights_count(void);
const char* genie_weights_name(int i);
int64_t genie_weights_numel(int i);
int64_t genie_weights_offset(int i);      /* offset (floats) of parameter i inside the flat mirror */
int64_t genie_weights_blob_floats(void);  /* size (floats) of the flat mirror; every offset is 16-B aligned */
int genie_weights_set(genie_ctx* ctx, const char* name, const float* dev_ptr, int64_t numel, void* stream);
/* Upload the whole mirror at once: `blob` holds every parameter at genie_weights_offset(i). */
int genie_weights_set_blob(genie_ctx* ctx, const float* blob_dev, int64_t n_floats, void* stream);
int genie_weights_commit(genie_ctx* ctx, void* stream);

/* Bytes of caller-provided workspace the forward calls need (256-B aligned base required). */
size_t genie_workspace_bytes(const genie_ctx* ctx);

/*
 * DataAggregation, stage 1 = everything that does not need the SECOND pair of neighbour means (module.py:87-95).
 * For every OWNED product node, with h0 = PReLU(init_trns([Slice || Mask])) recomputed on the fly for the node and
 * for each of its neighbours from their raw 8 input floats (h0 is never stored):
 *   h1 = PReLU1([l1_t1_2[h0||mean_sta PReLU11(h0)||M] || l1_t2_2[h0||mean_src PReLU12(h0)||M]])
 *   u = PReLU21(l2_t1_1 h1), v = PReLU22(l2_t2_1 h1)
 *   wu = l2_t1_2.weight[:, 60:90] u,  wv = l2_t2_2.weight[:, 60:90] v      (mean_N(W x) = W mean_N(x): the 15-channel
 *                                                                         operands the second pair of means averages)
 *   c  = [l2_t1_2.weight[:, 0:60] h1 + l2_t1_2.weight[:, 90:94] M + bias || same for l2_t2_2]   (node-local part)
 *   slice, mask : [n_grid_ext*n_sta, 4] fp32 — halo rows (sharded case) are shipped raw, 8 floats per row.
 * c, wu, wv are kept in the workspace; h1, u, v never leave the registers.
 */
int genie_da_stage1(genie_ctx* ctx, const float* slice, const float* mask, void* ws, void* stream);
/* Sub-range form for the source-node-sharded case (the halo exchange of `wv` overlaps compute): only the owned
 * source nodes at positions [gi_begin, gi_end) of the processing order (`grid_order` of genie_ctx_create) are processed.
 * `first` != 0 on the first range call of a window: it runs the input split pass over ALL rows (owned + halo); later range
 * calls of the same window (same slice / mask / workspace / slot) pass 0. A caller that puts the nodes other ranks need first
 * in the processing order can start sending their `wv` rows while the rest of stage 1 runs. */
int genie_da_stage1_range(genie_ctx* ctx, const float* slice, const float* mask, int gi_begin, int gi_end, int first,
                          void* ws, void* stream);
/* Parity/debug variant: additionally writes h0 [n_grid*n_sta, 30] and h1 [n_grid*n_sta, 60]. */
int genie_da_stage1_debug(genie_ctx* ctx, const float* slice, const float* mask, float* h0_out, float* h1_out,
                          void* ws, void* stream);
/*
 * Halo access for the sharded case: device pointer / row pitch (floats) of the projected `wv` activations
 * inside the workspace, laid out [n_grid_ext*n_sta, pitch] (pitch = 16: 15 channels + 1 zero); rows
 * >= n_grid*n_sta must be filled by the caller (RCCL) between stage 1 and stage 2.
 */
float* genie_ws_v_ptr(const genie_ctx* ctx, void* ws);
int genie_ws_v_pitch(const genie_ctx* ctx);
/*
 * DataAggregation stage 2 + BipartiteGraphOperator (module.py:94-96 and :224-229), OWNED rows:
 *   x_latent = PReLU2(c + [mean_sta wu || mean_src wv])                                      -> optional output
 *   out_g    = PReLU_b2(fc2( sum_s max_c(M) * PReLU_b1(fc1[x_latent || edge_attr]) ))       -> bip_out[n_grid,15]
 *   edge_attr : [n_grid*n_sta, 3] (`A_src_in_edges.x`, process_continuous_days.py:630)
 *   x_latent_out : [n_grid*n_sta, 30] or NULL when the caller does not need it (forward_fixed_source)
 */
int genie_da_stage2_bipartite(genie_ctx* ctx, const float* mask, const float* edge_attr,
                              float* x_latent_out, float* bip_out, void* ws, void* stream);
/* The two halves of genie_da_stage2_bipartite as separate calls (so they can sit on different streams):
 * per-tile station-sum partials (the P-sized kernel), then r_g = sum of partials and out_g = PReLU_b2(fc2 r_g). */
int genie_da_stage2_partials(genie_ctx* ctx, const float* mask, const float* edge_attr, float* x_latent_out, void* ws,
                             void* stream);
/* ... and the sub-range form of the P-sized half: partials of the owned source nodes at positions [gi_begin, gi_end) of the
 * processing order only. Nodes without halo neighbours can run before the halo rows of `wv` have arrived. */
int genie_da_stage2_partials_range(genie_ctx* ctx, const float* mask, const float* edge_attr, float* x_latent_out,
                                   int gi_begin, int gi_end, void* ws, void* stream);
int genie_bipartite_readout(genie_ctx* ctx, float* bip_out, void* ws, void* stream);
/*
 * SpatialAggregation (module.py:243-249; instances :889-891) on the source graph of this context.
 * Requires an UNSHARDED source graph (n_grid_ext == n_grid): when the product graph is sharded over source
 * nodes, the [G,15] Bipartite output is all-gathered and the three G-sized layers run on a second context
 * that holds the whole source graph (n_sta = 1).
 *   layer : 1, 2 or 3 (c_in = 15 for layer 1 else 30)
 *   x_in  : [n_grid, c_in], pos : [n_grid, 3] metres (divided by scale_rel inside, module.py:245)
 *   out   : [n_grid, 30]
 * The edge-mean of PReLU3(fglobal(x_j)) over ALL edges (module.py:249) is an out-degree weighted node mean.
 */
int genie_spatial_agg_fwd(genie_ctx* ctx, int layer, const float* x_in, const float* pos, float* out,
                          void* ws, void* stream);
/* SpatialAggregation1 -> 2 -> 3 chained (module.py:1012-1014): every layer kernel also emits the per-node pre-pass
 * of the next one (x-part of the message Linear and the edge-mean partials). x_in15 [n_grid,15] -> out [n_grid,30]. */
int genie_spatial_agg3_fwd(genie_ctx* ctx, const float* x_in15, const float* pos, float* out, void* ws, void* stream);

/*
 * Fused single-GPU path = module.py:1010-1014: DataAggregation -> Bipartite_ReadIn -> SpatialAggregation1..3.
 *   x_spatial_out : [n_grid, 30]; x_latent_out optional ([P,30] or NULL); bip_out optional ([n_grid,15] or NULL)
 */
int genie_path_fwd(genie_ctx* ctx, const float* slice, const float* mask, const float* edge_attr,
                   const float* pos, float* x_spatial_out, float* x_latent_out, float* bip_out,
                   void* ws, void* stream);

/*
 * Read-out heads needed to return (y, x) from forward_fixed_source (module.py:1015-1018).
 *   genie_readout_grid : y[n_grid, n_t]  = TemporalAttention(SpatialDirect(x_spatial), t_query)     module.py:251-260, 299-331
 *   genie_readout_query: x[n_query, n_t] = TemporalAttention(SpatialAttention(x_spatial, x_query, x_grid), t_query)
 *                        module.py:262-297; `knn` [n_query, 10] int32 = indices of the 10 nearest grid nodes of every
 *                        query (the `knn(x_context/1000, x_query/1000, k=10)` of module.py:282, computed by the caller
 *                        once per query set); softmax is over those 10 edges per head, aggregation 'add', mean over heads.
 *   x_spatial [n_grid,30]; x_grid [n_grid,3], x_query [n_query,3] in metres; t_query [n_t] seconds, n_t <= 10.
 */
int genie_readout_grid(genie_ctx* ctx, const float* x_spatial, const float* t_query, int n_t, float* y_out, void* stream);
int genie_readout_query(genie_ctx* ctx, const float* x_spatial, const float* x_grid, const float* x_query,
                        const int32_t* knn, int n_query, int k, const float* t_query, int n_t, float* x_out,
                        void* ws, void* stream);
/* Both read-outs of one window: y_out as genie_readout_grid, x_out as genie_readout_query (same arguments, same checks), bit-identical
 * to the two calls. Given x_spatial the heads are independent and each fills a fraction of the GPU, so after the per-grid-node table of
 * the query head both run in ONE launch, side by side on one stream. */
int genie_readouts(genie_ctx* ctx, const float* x_spatial, const float* x_grid, const float* x_query, const int32_t* knn,
                   int n_query, int k, const float* t_query, int n_t, float* y_out, float* x_out, void* ws, void* stream);
/* The same read-outs with the latent input of TemporalAttention exported next to them, as the 4-output forward needs it
 * (module.py:978-981): y_latent_out [n_grid, 30] = SpatialDirect(x_spatial) (:978), latent_out [n_query, 30] =
 * SpatialAttention(x_spatial, x_query, x_grid) (:981, `x_src` for the candidate sources). */
int genie_readout_grid_latent(genie_ctx* ctx, const float* x_spatial, const float* t_query, int n_t, float* y_out,
                              float* y_latent_out, void* stream);
int genie_readout_query_latent(genie_ctx* ctx, const float* x_spatial, const float* x_grid, const float* x_query,
                               const int32_t* knn, int n_query, int k, const float* t_query, int n_t, float* x_out,
                               float* latent_out, void* ws, void* stream);

/*
 * Pick -> Slice/Mask embedding on device = `extract_input_from_data` (process_utils.py:460-642, use_sign_input False),
 * the step that feeds the path once per window. Removes the [P,8] fp32 H2D copy per window.
 *   pick_t [n] float64 absolute pick times, pick_sta [n] int32 station index in the model's station order (-1 = not
 *   used), pick_phase [n] int32 (0 = P, 1 = S); the caller passes the picks inside (t0 - 2 sigma, t0 + max_t + 2 sigma)
 *   (process_utils.py:476). trv [n_grid_ext*n_sta, 2] fp32 theoretical P / S travel times per product node (static).
 *   emb_ws: scratch of 2 * n_sta * genie_embed_ntime(...) floats. Outputs slice_out / mask_out [n_grid_ext*n_sta, 4].
 */
int genie_embed_ntime(double t0, double max_t, double kernel_sig_t, double dt);
int genie_embed_window(genie_ctx* ctx, const double* pick_t, const int32_t* pick_sta, const int32_t* pick_phase, int n_picks,
                       double t0, double max_t, double kernel_sig_t, double dt, const float* trv, float* emb_ws,
                       float* slice_out, float* mask_out, void* stream);
/* Same, and additionally leaves the split input rows of the f16x2 stage-1 kernel in `workspace`: the NEXT genie_da_stage1 /
 * genie_path_fwd call on this context with exactly these slice_out / mask_out pointers and this workspace skips its
 * k_split_rows pass (one-shot; the caller must not modify Slice / Mask in between, and stage 1 must run on the same stream or
 * after it). A no-op extension on contexts that do not use the f16x2 kernel. */
int genie_embed_window_split(genie_ctx* ctx, const double* pick_t, const int32_t* pick_sta, const int32_t* pick_phase,
                             int n_picks, double t0, double max_t, double kernel_sig_t, double dt, const float* trv,
                             float* emb_ws, float* slice_out, float* mask_out, void* workspace, void* stream);

/* Neighbour means on the implicit product graph for [P, row_floats] fp32 rows (row_floats = 16 or 32, 16-byte aligned, or 30 = unpadded [P, 30] rows, 8-byte aligned):
 *   out_sta[(g,s)] = mean_k x_sta[(g, sta_nbr_k(s))]      (MessagePassing('mean') over A_in_sta)
 *   out_src[(g,s)] = mean_k x_src[(src_nbr_k(g), s)]      (... over A_in_src; x_src has n_grid_ext * n_sta rows)
 * Either pair may be null; an empty neighbourhood gives 0. A stand-alone building block (the means of
 * DataAggregationAssociationPhase, module.py:395-400, for a caller who keeps the per-node Linears in PyTorch): the fused
 * association kernels of this library do not call it. */
int genie_nbr_mean(genie_ctx* ctx, const float* x_sta, const float* x_src, float* out_sta, float* out_src, int row_floats,
                   void* stream);
/* Backward of a single-slope PReLU over n contiguous fp32 values (training path): dx = x > 0 ? dy : slope * dy
 * (torch.nn.functional.prelu's backward: the slope applies at x == 0, of either sign), dslope[0] = sum over x <= 0 of dy * x (the
 * terms at zero add nothing), summed in a fixed order. `scratch` = 2048 floats; pointers 16-byte aligned. */
int genie_prelu_bwd(const float* x, const float* dy, const float* slope, int64_t n, float* dx, float* dslope, float* scratch,
                    void* stream);

/* Weight and bias gradients of a per-node Linear y = x W^T + b over N contiguous rows (training path):
 * dW[M, K] = dy^T x, db[M] = column sums of dy (db may be NULL), M <= 128, K <= 128, summed in a fixed order.
 * `scratch` holds genie_linear_bwd_scratch_floats(K) floats. */
int64_t genie_linear_bwd_scratch_floats(int K);
int genie_linear_bwd_wb(const float* x, const float* dy, int64_t N, int K, int M, float* dW, float* db, float* scratch, void* stream);

/* Adjoint of genie_nbr_mean (training): dx_sta[(g,j)] = sum_{i : j in N_sta(i)} g_sta[(g,i)] / deg(i), likewise for the source
 * graph. Deterministic (a gather over the reversed graphs, built once per context); unsharded Cartesian contexts only. */
int genie_nbr_mean_bwd(genie_ctx* ctx, const float* g_sta, const float* g_src, float* dx_sta, float* dx_src, int row_floats,
                       void* stream);

/* out_dev [n_blocks][2] = (HW_REG_XCC_ID, HW_REG_HW_ID) of the CU every workgroup of a probe launch ran on: workgroup b of a
 * launch lands on XCD b % 8, which the XCD-chunked sweeps of the stage kernels rely on (for speed only). */
int genie_where_am_i(int32_t* out_dev, int n_blocks, void* stream);
/* Grid caps (workgroups) of the read-out (k_readout, k_ro_pre) and SpatialAggregation kernels of the G-sized tail; 0 = default
 * (one read-out workgroup per CU, two SpatialAggregation workgroups per CU: lowest latency). In the window pipeline, where a
 * tail workgroup has a CU to itself while it lives, fewer workgroups cost the P-sized kernels less CU-time as long as the
 * tail chain still ends within two windows: 96 / 64 at config 2 on 256 CUs is 3.4 % faster end to end, 64 / 32 is 9 % slower. */
int genie_set_tail_grid(genie_ctx* ctx, int readout_workgroups, int sa_workgroups);

/* Training step of the path (train_GENIE_model.py:1786-1861): DataAggregation + the P-sized half of
 * Bipartite_ReadIn forward with the pre-activations kept, and their backward as three P-sized HIP passes.
 *   genie_da_train_fwd: the generic fp32 stage kernels (same arithmetic as genie_da_stage1 / genie_da_stage2_partials) with
 *     `save` (genie_train_save_floats(ctx) floats) filled; x_latent_out [P, 30] optional; r_out [n_grid, 30] = the per-source-
 *     node station sum of the gated Bipartite messages (module.py:229, before fc2: out_g = PReLU_b2(fc2 r_g) stays with the
 *     caller, G-sized).
 *   genie_da_train_bwd: d_r [n_grid, 32] (gradient of r_out, rows padded to 32 floats) -> grad_blob: gradients of every
 *     DataAggregation parameter and of Bipartite_ReadIn.fc1 / activate1, laid out like the weight mirror
 *     (genie_weights_offset(i), genie_weights_blob_floats() floats; entries of other parameters are zero). `scratch`:
 *     genie_train_scratch_floats(ctx) floats. Deterministic (fixed-order reduction of per-wave partials).
 * Unsharded product graphs, Cartesian or irregular (genie_ctx_create_subgraph: tiles of 16 consecutive product nodes, the transposed
 * means of the backward over the reversed PRODUCT-level graphs; round 4). With genie_set_edge_features / genie_set_absolute_pos in force (the two other model
 * definitions) the forward is those variants' inference kernels and the backward adds the gradients of their static-term weights
 * ("<layer>.weight_pos", "init_trns.weight_abs"): such a term is W_f f[n] with f a fixed table over the stations or the source
 * nodes, so dW_f = sum_n (sum of the kept gradient rows over the product nodes of n) (x) f[n] -- per-station / per-source-node
 * sums of the rows the three passes keep (k_gr_sum_sta / k_gr_sum_src), contracted with the table (k_static_dw), fixed order. */
size_t genie_train_save_floats(const genie_ctx* ctx);
size_t genie_train_scratch_floats(const genie_ctx* ctx);
int genie_da_train_fwd(genie_ctx* ctx, const float* slice, const float* mask, const float* edge_attr, float* save,
                       float* x_latent_out, float* r_out, void* ws, void* stream);
int genie_da_train_bwd(genie_ctx* ctx, const float* slice, const float* mask, const float* edge_attr, const float* save,
                       const float* d_r, float* scratch, float* grad_blob, void* stream);

/* Training step, the G- / Q-sized tail (round 3): Bipartite_ReadIn.fc2 (module.py:229), SpatialAggregation1..3 (:243-249, the
 * grid-wide edge-mean term included), SpatialDirect (:251-260), SpatialAttention (:262-297) and TemporalAttention (:299-331,
 * applied to both read-outs), i.e. everything of `forward_fixed_source` (:1011-1018) after the station sum, in both directions.
 *   genie_tail_train_fwd: call right after genie_da_train_fwd on the same workspace slot (it consumes the per-tile partials).
 *     It IS the inference tail (k_bip_out_m, k_sa_pre_m / k_sa_layer_m, k_ro_pre_m, k_readout_m); the layer inputs the backward
 *     recomputes from (r, bip, sa1, sa2, x_spatial) go to `tsave` (genie_tail_train_save_floats(ctx) floats; x_spatial [n_grid, 30]
 *     starts at float 112 * n_grid). y_out [n_grid, n_t], x_out [n_query, n_t]; y_latent_out [n_grid, 30] optional
 *     (SpatialDirect output, the input of the association heads).
 *   genie_tail_train_bwd: d_y [n_grid, n_t], d_x [n_query, n_t]; optional extra upstream gradients d_xs_extra [n_grid, 30]
 *     (other consumers of x_spatial), d_ylat_extra [n_grid, 30] (other consumers of y_latent) and d_qlat_extra [n_query, 30] (consumers
 *     of the SpatialAttention output of a query row, :981: the `x_src` rows the arrival head reads) -> d_r_out [n_grid, 32] (the
 *     input of genie_da_train_bwd) and grad_blob (genie_train_grad_floats() floats, zeroed by the call; weight-mirror layout):
 *     gradients of every tail parameter. rknn_rowptr [n_grid + 1] / rknn_edge [n_query * 10]: the query kNN table reversed =
 *     for every grid node the attention edges i * 10 + k that end in it, ascending. `scratch`:
 *     genie_tail_train_scratch_floats(ctx, n_query) floats. Deterministic: per-wave partial sums reduced in a fixed order,
 *     scatter-shaped gradients gathered over reversed graphs, no atomics.
 *   genie_train_bwd: genie_tail_train_bwd followed by genie_da_train_bwd (driven by the tail's d r) into ONE gradient blob:
 *     the whole backward of a `forward_fixed_source` training step (train_GENIE_model.py:1843-1846). */
size_t genie_tail_train_save_floats(const genie_ctx* ctx);
size_t genie_tail_train_scratch_floats(const genie_ctx* ctx, int n_query);
size_t genie_train_grad_floats(void);
int genie_tail_train_fwd(genie_ctx* ctx, const float* pos, const float* x_query, const int32_t* knn, int n_query, int k,
                         const float* t_query, int n_t, float* tsave, float* y_latent_out, float* y_out, float* x_out, void* ws,
                         void* stream);
int genie_tail_train_bwd(genie_ctx* ctx, const float* pos, const float* x_query, const int32_t* knn, const int32_t* rknn_rowptr,
                         const int32_t* rknn_edge, int n_query, int k, const float* t_query, int n_t, const float* tsave,
                         const float* d_y, const float* d_x, const float* d_xs_extra, const float* d_ylat_extra, const float* d_qlat_extra,
                         float* scratch, float* d_r_out, float* grad_blob, void* stream);
int genie_train_bwd(genie_ctx* ctx, const float* slice, const float* mask, const float* edge_attr, const float* save, const float* pos,
                    const float* x_query, const int32_t* knn, const int32_t* rknn_rowptr, const int32_t* rknn_edge, int n_query, int k,
                    const float* t_query, int n_t, const float* tsave, const float* d_y, const float* d_x, const float* d_xs_extra,
                    const float* d_ylat_extra, const float* d_qlat_extra, float* tail_scratch, float* front_scratch, float* d_r_scratch,
                    float* grad_blob, void* stream);

/* Association heads on the product graph, the P-sized part of `forward_fixed` after the source branch
 * (module.py:986-990): BipartiteGraphReadOutOperator (:333-352) followed by DataAggregationAssociationPhase (:356-403).
 *   y_latent [n_grid, 30] (SpatialDirect output), mask_src [n_grid] (`mask_out`, :985), x_latent [P, 30] (DataAggregation
 *   output, detached at :990), mask [P, 4], edge_attr [P, 3]  ->  out [P, 30]
 * assoc_ws: genie_assoc_workspace_bytes(ctx) bytes of scratch (16-byte aligned; tr / q1 rows [P][32], q2 rows [P_ext][32]). The call reuses the c / wu /
 * wv buffers of the current workspace slot: issue it after the DataAggregation stage 2 of the same window. Parameters under
 * their state_dict names ("BipartiteGraphReadOutOperator.*", "DataAggregationAssociationPhase.*"; the static-term columns of the two
 * other model definitions under "<name>_pos" / "<name>_abs", as for DataAggregation).
 * Unsharded product graphs (Cartesian, or irregular since round 4: product-level CSR forms of the kernels). */
size_t genie_assoc_workspace_bytes(const genie_ctx* ctx);
int genie_assoc_fwd(genie_ctx* ctx, const float* y_latent, const float* mask_src, const float* x_latent, const float* mask,
                    const float* edge_attr, float* out, void* assoc_ws, void* ws, void* stream);

/* genie_assoc_fwd on a source-node shard (a context with n_grid_ext > n_grid; Cartesian product graphs), cut where a layer gathers rows
 * of neighbouring source nodes, which for the halo nodes another rank computes. Same arguments; y_latent / mask_src are the rows of the
 * OWNED source nodes in local order, x_latent / mask / edge_attr / out the owned product-node rows [n_grid * n_sta, .].
 *   part 0: the per-node front (k_assoc_pre, k_assoc_a) over the owned rows. Leaves q2, the operand of layer 1's source-side mean, in
 *           assoc_ws: [n_grid_ext * n_sta][32] floats at byte offset genie_assoc_halo_offset(ctx) - 128 * n_grid * n_sta, owned rows first.
 *           The caller fills the halo rows (from genie_assoc_halo_offset(ctx) on, halo order) with their owners' rows before part 1.
 *   part 1: layer 1 and the node-local half of layer 2 (k_assoc_b) over the owned rows; reads q2 in the extended row space. Leaves
 *           layer 2's gather operand in the workspace's wv rows (genie_ws_v_ptr), whose halo rows the caller fills before part 2.
 *   part 2: the second pair of neighbour means (the stage-2 kernel) -> out.
 * A node's neighbour rows are accumulated in the order of its in-edges, as genie_assoc_fwd does: the result does not depend on how the
 * source nodes are split. On an unsharded context the three parts in sequence are genie_assoc_fwd. */
size_t genie_assoc_halo_offset(const genie_ctx* ctx);
int genie_assoc_fwd_part(genie_ctx* ctx, int part, const float* y_latent, const float* mask_src, const float* x_latent, const float* mask,
                         const float* edge_attr, float* out, void* assoc_ws, void* ws, void* stream);

/* Exact k nearest neighbours on the device, replacing the reference's `torch_cluster.knn(x_context / scale, x_query / scale, k)`
 * calls: out_idx [n_query, k] int32 = indices into x_context of the k nearest context points of every query, nearest first
 * (ties: smaller index first; -1 when fewer than k candidates exist). fp64 distances on the fp32 coordinates as given: the
 * reference's common factor 1 / 1000 (module.py:282, process_utils.py:718-719) does not change the order. exclude_self != 0: candidate i is skipped for query
 * i (x_query = x_context: the `knn(x, x, k + 1)` + `remove_self_loops` idiom of the base graphs). 1 <= k <= 16. */
int genie_knn(const float* x_context, int n_context, const float* x_query, int n_query, int k, int exclude_self,
              int32_t* out_idx, void* stream);

/* The same table through a cell index of the context points, for large query sets against a context that stays (the refine pass's
 * 112 000-point cloud per candidate source against the source grid): EXACT -- out_idx of genie_knn_indexed equals out_idx of genie_knn
 * on the same points bit for bit, ties and -1 entries included -- and opt-in; genie_knn is unchanged.
 *   The index is a uniform cell grid over the bounding box of the context points (fp32 coordinates as passed): the cell edge gives a
 *   mean occupancy of 4 points per cell, at most 2^20 cells, one cell on an axis of zero extent; cell id = (c2 * cells[1] + c1) *
 *   cells[0] + c0 with c_a = clamp(floor(fl(fl(x_a - origin[a]) * inv_cell)), 0, cells[a] - 1) in fp32. Its buffers are the caller's:
 *   cell_start int32 [n_cells + 1] and records [n_context] of 16 bytes (x, y, z, bits of the original index; 16-byte aligned), the
 *   points ordered by cell.
 * genie_knn_index_plan: host only, no device call. bbox = (min x, y, z, max x, y, z) -> the cells per axis, the cell function's
 *   constants and the byte sizes of the buffers. A box that is not finite returns GENIE_ERR_ARG.
 * genie_knn_index_build, two passes as the count / fill pairs of this header. Pass 1 (cell_start == NULL): the bounding box on the
 *   device into bbox_dev (device, 6 floats), read back once (this pass waits for the stream), and *plan filled from it; a context with
 *   a NaN or an infinity returns GENIE_ERR_ARG here. Pass 2 (the buffers of that plan; scratch = device int32 [n_cells], left as the
 *   cells' counts): cell ids, histogram, exclusive scan, scatter, on the stream, no wait.
 * genie_knn_indexed: the arguments of genie_knn with (cell_start, records, plan, n_context) in place of the context. One lane per
 *   query; a query outside the box starts in the nearest cell. */
typedef struct genie_knn_index_plan_t {
    int32_t cells[3];
    int32_t n_cells;             /* cells[0] * cells[1] * cells[2] <= 2^20 */
    float origin[3];             /* lower corner of the bounding box */
    float upper[3];              /* upper corner */
    float inv_cell;              /* fp32 factor of the cell function */
    int32_t reserved;
    double cell;                 /* cell edge = 1 / (double)inv_cell */
    int64_t cell_start_bytes;    /* 4 * (n_cells + 1) */
    int64_t records_bytes;       /* 16 * n_context */
    int64_t scratch_bytes;       /* 4 * n_cells */
} genie_knn_index_plan_t;
int genie_knn_index_plan(int n_context, const float* bbox, genie_knn_index_plan_t* plan);
int genie_knn_index_build(const float* x_context, int n_context, float* bbox_dev, genie_knn_index_plan_t* plan, int32_t* cell_start,
                          float* records, int32_t* scratch, void* stream);
int genie_knn_indexed(const int32_t* cell_start, const float* records, const genie_knn_index_plan_t* plan, int n_context,
                      const float* x_query, int n_query, int k, int exclude_self, int32_t* out_idx, void* stream);

/* One-time graph setup, training call convention (round 5): `forward` receives the product edge lists of a NEW graph per sample
 * (train_GENIE_model.py:1722-1786; built at :1140-1149 as process_utils.py:720-721 builds them) and the library consumes only their base
 * graphs, so every sample's lists are verified to be the Cartesian product of their own first blocks:
 *   A_in_sta int64 [2][E_sta] (row 0 then row 1), E_sta = n_grid * e_sta, entry e = base_sta[e % e_sta] + n_sta * (e / e_sta);
 *   A_in_src int64 [2][E_src], E_src = n_sta * e_src, entry e = base_src[e % e_src] + (e / e_src), base_src multiples of n_sta.
 * `flags` (device int32, zeroed by the caller) gets bit 0 set when A_in_sta is not of that form, bit 1 when A_in_src is not. One pass,
 * no allocation, no synchronisation (replaces the `torch.equal` of two materialised copies in genie_amd/graph.py). */
int genie_product_check(const int64_t* A_in_sta, int64_t E_sta, const int64_t* A_in_src, int64_t E_src, int n_sta, int n_grid,
                        int32_t* flags, void* stream);

/* Training step of the P-sized association heads (round 3; module.py:986-990 inside train_GENIE_model.py:1786-1861):
 *   genie_assoc_train_fwd = genie_assoc_fwd in the caller's station order with the pre-activations of every layer kept in `asave`
 *     (genie_assoc_train_save_floats(ctx) floats: 20 blocks of 16 floats per product node);
 *   genie_assoc_train_bwd: d_s [P, 30] (gradient of the head's output) -> d_ylat_out [n_grid, 30] (gradient of y_latent; x_latent is
 *     detached at module.py:990) and grad_blob (genie_weights_blob_floats() floats, zeroed by the call, weight-mirror layout): gradients of
 *     every BipartiteGraphReadOutOperator / DataAggregationAssociationPhase parameter. Four P-sized passes (k_as_b3, k_train_b1<true>,
 *     k_as_b1, k_as_b0: the structure of DataAggregation's backward) + one G-sized (k_as_g); `scratch`:
 *     genie_assoc_train_scratch_floats(ctx) floats. Deterministic. Unsharded product graphs, Cartesian or irregular; under the two other model
 *     definitions the static-term weight gradients are added as in genie_da_train_bwd. */
size_t genie_assoc_train_save_floats(const genie_ctx* ctx);
size_t genie_assoc_train_scratch_floats(const genie_ctx* ctx);
int genie_assoc_train_fwd(genie_ctx* ctx, const float* y_latent, const float* mask_src, const float* x_latent, const float* mask,
                          const float* edge_attr, float* out, float* asave, void* assoc_ws, void* ws, void* stream);
int genie_assoc_train_bwd(genie_ctx* ctx, const float* y_latent, const float* mask_src, const float* x_latent, const float* mask,
                          const float* edge_attr, const float* asave, const float* d_s, float* scratch, float* d_ylat_out,
                          float* grad_blob, void* stream);

/* LocalSliceLgCollapse P (phase_head 0) / S (1), module.py:610-659, on the device: for every pick the 10 product nodes listed in the
 * time-pointer table a_edges [n_sta * l_dt * 10] (int32 product-node ids, `assemble_time_pointers_for_stations`, utils.py:602-622)
 * at (ipick, floor((tpick - t0) / dt)), those with |tpick - tlatent[e * tl_stride + tl_col]| < 2 eps kept, edge MLP on the rows of
 * s_rows [P, 30] (genie_assoc_fwd), mean, fc2: out [n_picks, 15]. t0 = dt_partition[0], dt = dt_partition[1] - dt_partition[0]: either
 * passed as numbers (dt_partition NULL) or read by the kernel from the caller's DEVICE array dt_partition [l_dt >= 2] (t0 / dt ignored:
 * a caller holding the partition on the device needs no read-back). tpick / phase_label fp32 [n_picks], ipick int32. An index outside
 * the table is clamped and reported through genie_index_flags. */
int genie_lslc_fwd(genie_ctx* ctx, int phase_head, const float* s_rows, const int32_t* a_edges, int64_t n_edges, int l_dt, float t0,
                   float dt, const float* dt_partition, float eps, const float* tlatent, int tl_stride, int tl_col, const float* tpick,
                   const int32_t* ipick, const float* phase_label, int n_picks, float* out, void* stream);

/* genie_lslc_fwd on a source-node shard, in two halves around one all-gather: the rows of `s` a pick's table entry points to live with
 * the ranks that own their source nodes.
 * genie_lslc_rows (on the shard's context): the lookup of genie_lslc_fwd for BOTH heads. s_own [n_grid * n_sta, 30] = the association
 * embedding of the owned source nodes (local node order), node_local int32 [n_grid_all]: global source node -> local owned index or -1,
 * a_edges_p / a_edges_s [n_edges] the two tables (GLOBAL product-node ids), tlatent [n_grid_all * n_sta][tl_stride] with the P / S
 * arrival in columns 0 / 1. For every entry (head, pick, slot) whose product node this rank owns, one row of 32 floats is appended to
 * `rows` (room for 2 * n_picks * 10 rows): [0:30] the s row, [30] its theoretical arrival, [31] the BITS of the int32 entry number
 * (head * n_picks + pick) * 10 + slot. count [1] int32 = rows written (zeroed by the call). The order of the list is unspecified; an
 * index outside the table is clamped and reported through genie_index_flags as genie_lslc_fwd does, so is a table entry that is no
 * product node (which no rank owns).
 * genie_lslc_fwd_rows (on any context with the head's parameters): the rest of genie_lslc_fwd on table [2 * n_picks * 10][32], the
 * ranks' rows placed at their entry numbers (every entry has one owner: place, never add). */
int genie_lslc_rows(genie_ctx* ctx, const float* s_own, const int32_t* node_local, int n_grid_all, const int32_t* a_edges_p,
                    const int32_t* a_edges_s, int64_t n_edges, int l_dt, float t0, float dt, const float* dt_partition, const float* tlatent,
                    int tl_stride, const float* tpick, const int32_t* ipick, int n_picks, int32_t* count, float* rows, void* stream);
/* genie_lslc_rows for a rank that holds the travel times of its owned rows only (tables built by genie_time_pointers_candidates /
 * _merge): tlatent_own [n_own * n_sta][tl_stride] (n_own = the context's n_grid) in the local node order of s_own. The arrival of a listed row is read where its s row
 * is, on the rank that owns it, and travels in column 30 of the same compact row: the lists, and the one all-gather, are unchanged. */
int genie_lslc_rows_own(genie_ctx* ctx, const float* s_own, const int32_t* node_local, int n_grid_all, const int32_t* a_edges_p,
                        const int32_t* a_edges_s, int64_t n_edges, int l_dt, float t0, float dt, const float* dt_partition,
                        const float* tlatent_own, int tl_stride, const float* tpick, const int32_t* ipick, int n_picks, int32_t* count,
                        float* rows, void* stream);
int genie_lslc_fwd_rows(genie_ctx* ctx, int phase_head, const float* table, float eps, const float* tpick, const float* phase_label,
                        int n_picks, float* out, void* stream);

/* Backward of genie_lslc_fwd for training steps (round 3; k_lslc_bwd, forward recomputed per tile): d_out [n_picks, 15] -> the head's
 * fc1 / fc2 / PReLU-slope gradients ADDED into grad_blob (weight-mirror layout; zero it once before the two heads), the gradient of every
 * gathered s row in erow [n_picks * 10][32] and its product node in etgt [n_picks * 10] (-1 = dropped by the 2-eps filter, module.py:642-647).
 * genie_seg_rows adds those rows into d_s [P, 30] per product node, in the order of `order` (the edges sorted by etgt, stable): several
 * picks may gather the same node, and the sum must not depend on scheduling. part_scratch: genie_lslc_bwd_part_floats(n_picks) floats. */
size_t genie_lslc_bwd_part_floats(int n_picks);
int genie_lslc_bwd(genie_ctx* ctx, int phase_head, const float* s_rows, const int32_t* a_edges, int64_t n_edges, int l_dt, float t0,
                   float dt, const float* dt_partition, float eps, const float* tlatent, int tl_stride, int tl_col, const float* tpick,
                   const int32_t* ipick, const float* phase_label, int n_picks, const float* d_out, float* erow, int32_t* etgt,
                   float* part_scratch, float* grad_blob, void* stream);
int genie_seg_rows(const float* erow, const int32_t* etgt, const int32_t* order, int64_t n_edges, float* d_s, void* stream);

/* StationSourceAttentionMergedPhases (`Arrivals`, module.py:662-775; use_sparse = True, use_neighbor_assoc_edges = False) on
 * the device: out [n_src, n_arv, 2]. stime [n_src] (`tq_sample`), src_embed [n_src, 30] (`x_src`), trv_src [n_src, n_sta, 2]
 * (`trv_out_q`), arrival_p / arrival_s [n_arv, 15] (genie_lslc_fwd), tpick / phase_label fp32 [n_arv]. The picks grouped by station:
 * order [n_arv] = pick ids sorted by station (stable), and for each of the n_useg stations that have picks its id, the start of
 * its picks in `order` and their count. ctx_scratch: n_src * 192 floats; e0max_scratch: one int32 where the call leaves
 * `edge_index[0].max()` over the kept edges (:762-763), the pick index the reference uses for `self_link` / `null_link` (:764-765):
 * the null pick n_arv whenever some source has |stime| < 2 eps (the null pick of :715-718 then survives the time filter), otherwise
 * the largest pick index with a kept edge -- reproduced as the reference computes it. The segment softmax (:773) runs in streaming
 * form over chunks of 192 picks of a station, so a station may hold any number of picks. */
int genie_arrivals_fwd(genie_ctx* ctx, int n_src, const float* stime, const float* src_embed, const float* trv_src, int n_sta,
                       const float* arrival_p, const float* arrival_s, const float* tpick, const float* phase_label, int n_arv,
                       const int32_t* order, const int32_t* seg_sta, const int32_t* seg_start, const int32_t* seg_len, int n_useg,
                       float eps, float* ctx_scratch, int32_t* e0max_scratch, float* out, void* stream);

/* The same head inside a training step (train_GENIE_model.py:1786-1861 differentiates module.py:662-775). _train_fwd = the forward
 * above that also keeps, per (source, pick), the three normalised head aggregates and the softmax statistics in `save`
 * (genie_arrivals_train_save_floats(n_src, n_arv) floats); ctx_scratch / e0max_scratch must be kept for the backward as well.
 * genie_arrivals_bwd: d_out [n_src, n_arv, 2] -> d_src_embed [n_src, 30], d_arrival_p / d_arrival_s [n_arv, 15], and the gradients of
 * the head's 24 parameters ADDED into grad_blob (registry layout, genie_train_grad_floats() floats; the f_src_context_* entries are
 * written). The reference's per-call edge list is never built: queries / values are functions of (pick, source) and the two link
 * bits, so the backward is one pointwise pass over the (source, pick) targets (proj_1 / proj_2, d aggregate, the softmax's segment
 * term in closed form), one pass over the (source, station) pairs (forward of every entry recomputed, one sweep over the station's
 * targets, the edge MLPs backwards), and a per-source pass for the context MLP. No atomics, fixed summation order: bitwise
 * reproducible. scratch: genie_arrivals_bwd_scratch_floats(n_src, n_arv, n_useg) floats. */
int64_t genie_arrivals_train_save_floats(int n_src, int n_arv);
int genie_arrivals_train_fwd(genie_ctx* ctx, int n_src, const float* stime, const float* src_embed, const float* trv_src, int n_sta,
                             const float* arrival_p, const float* arrival_s, const float* tpick, const float* phase_label, int n_arv,
                             const int32_t* order, const int32_t* seg_sta, const int32_t* seg_start, const int32_t* seg_len, int n_useg,
                             float eps, float* ctx_scratch, int32_t* e0max_scratch, float* out, float* save, void* stream);
int64_t genie_arrivals_bwd_scratch_floats(int n_src, int n_arv, int n_useg);
int genie_arrivals_bwd(genie_ctx* ctx, int n_src, const float* stime, const float* src_embed, const float* trv_src, int n_sta,
                       const float* arrival_p, const float* arrival_s, const float* tpick, const float* phase_label, int n_arv,
                       const int32_t* order, const int32_t* seg_sta, const int32_t* seg_start, const int32_t* seg_len, int n_useg,
                       float eps, const float* ctx_scratch, const int32_t* e0max_scratch, const float* save, const float* d_out,
                       float* scratch, float* d_src_embed, float* d_arrival_p, float* d_arrival_s, float* grad_blob, void* stream);

/* Product-level CSRs of the irregular product graph of `use_subgraph: True` on the device (the two `subgraph(...)` loops of
 * extract_inputs_adjacencies_subgraph, process_utils.py:824-839). Product node n = the pair (pair_sta[n], pair_src[n]), pairs
 * sorted by (source, station) (:790-794); seg_rowptr[g] .. seg_rowptr[g+1] = the nodes of source node g; (sta_rowptr, sta_col) /
 * (src_rowptr, src_col) = in-edge CSRs of the base kNN graphs (:782-783). Two passes: _count fills the in-degrees
 * count_sta[n_prod] / count_src[n_prod]; the caller scans them into p_*_rowptr[n_prod + 1] (int32) and allocates the column
 * arrays; _fill writes the neighbours in base edge order. The results feed genie_ctx_create_subgraph directly. */
int genie_subgraph_csr_count(const int32_t* pair_sta, const int32_t* pair_src, int64_t n_prod, const int32_t* seg_rowptr,
                             const int32_t* sta_rowptr, const int32_t* sta_col, const int32_t* src_rowptr, const int32_t* src_col,
                             int32_t* count_sta, int32_t* count_src, void* stream);
int genie_subgraph_csr_fill(const int32_t* pair_sta, const int32_t* pair_src, int64_t n_prod, const int32_t* seg_rowptr,
                            const int32_t* sta_rowptr, const int32_t* sta_col, const int32_t* src_rowptr, const int32_t* src_col,
                            const int32_t* p_sta_rowptr, const int32_t* p_src_rowptr, int32_t* p_sta_col, int32_t* p_src_col,
                            void* stream);

/* Downstream reduction of the apply loop on the device (process_continuous_days.py:812-849): select entries of the stacked
 * output x [rows, cols] (fp32, row-major, e.g. Out_2 [n_query, len(tsteps_abs)]) without copying it to the host.
 *   mode 0: x > threshold                       = `np.where(Out_2 > 0.01)` (:812-813), row-major order
 *   mode 1: local maxima of every row with x >= threshold = scipy.signal.find_peaks(row, height = threshold) BEFORE its
 *           distance filter (:846): strict maxima and midpoints of flat tops, never the first / last sample
 * Two passes: genie_row_select_count fills counts[rows]; the caller turns them into exclusive offsets[rows] (int64) and
 * allocates the outputs; genie_row_select_fill writes (row, col, value) triplets in row-major order. */
int genie_row_select_count(const float* x, int rows, int64_t cols, float threshold, int mode, int32_t* counts, void* stream);
int genie_row_select_fill(const float* x, int rows, int64_t cols, float threshold, int mode, const int64_t* offsets,
                          int32_t* out_row, int32_t* out_col, float* out_val, void* stream);

/* Source detection after the peaks, on the device (process_continuous_days.py:846-891; LocalMarching, process_utils.py:40-100).
 * The host functions of genie_amd/postproc.py are the oracle of all three; flags are uint8 (1 = kept).
 *
 * genie_peak_distance: the distance rule of scipy.signal.find_peaks on the triplets genie_row_select_fill (mode 1) wrote.
 *   offsets [rows] are the exclusive row offsets handed to it, n the number of triplets, d = ceil(distance) >= 1. Walking from the
 *   highest peak of a row down, a kept peak removes every peak of the row closer than d columns; of two EQUAL heights within d the later
 *   column wins (scipy leaves that case to an unstable sort). keep [n].
 * genie_time_groups: t [n] ascending (fp64); node i starts a new group when t[i] - t[i - 1] >= break_win; group [n] = number of starts
 *   up to and including i (0 for the first group); break_win finite. scratch: genie_time_groups_scratch_ints(n) int32.
 * genie_local_marching: n nodes SORTED BY TIME (the caller's contract, not checked): xs [n, 3] fp64 positions already mapped and
 *   depth-scaled, t [n] fp64, val [n] fp32, group [n] or NULL (one group). j is an in-neighbour of i when both are in the same group,
 *   (t_i - t_j)^2 <= tc_win^2 and ((dx0^2 + dx1^2) + dx2^2) <= sp_win^2 (fp64, inclusive, unfused); a node with no neighbour but itself
 *   is kept as it is; the others take the maximum over their in-neighbours (use_directed: only those with val[i] <= val[j]) for
 *   n_steps_max steps or until a step changes nothing by more than tol, and survive when |val - marched| <= 1e-8 + tol |marched| (fp32).
 *   scratch: genie_local_marching_scratch_bytes(n) bytes, 16-byte aligned. keep [n]. Values must not be NaN.
 * Bad arguments (n < 0, a null pointer with n > 0, d < 1, tc_win / sp_win negative or not finite) return GENIE_ERR_ARG before any launch. */
int genie_peak_distance(const int64_t* offsets, int rows, int64_t n, const int32_t* col, const float* val, int d, uint8_t* keep,
                        void* stream);
int64_t genie_time_groups_scratch_ints(int64_t n);
int genie_time_groups(const double* t, int64_t n, double break_win, int32_t* scratch, int32_t* group, void* stream);
size_t genie_local_marching_scratch_bytes(int64_t n);
int genie_local_marching(const double* xs, const double* t, const float* val, const int32_t* group, int64_t n, double tc_win,
                         double sp_win, int n_steps_max, double tol, int use_directed, void* scratch, uint8_t* keep, void* stream);

/* Peak candidates of a column band of Out_2 (window-parallel days that keep Out_2 distributed, genie_amd/postproc.py::
 * detect_sources_banded): band [rows, width] fp32 with row stride `stride` (elements) holds the global columns [b_lo, b_lo + width) of an
 * axis of n_cols columns. Written are the mode-1 peaks of the row selection above -- local maxima >= threshold, flat tops at their
 * midpoint, never global column 0 or n_cols - 1 -- whose reported column lies in the own range [o_lo, o_hi): triplets (row, GLOBAL column, value),
 * row-major, columns ascending within a row, the same two passes as the row selection: counts [rows] -> the caller's exclusive int64
 * offsets [rows] -> fill. Own ranges that partition the axis report every peak of the full matrix exactly once.
 * A flat top is followed to both of its ends inside the band. One that reaches an end of the band which is not an end of the axis, and
 * whose midpoint could fall into the own range, cannot be decided from the band: *flag (int32, zeroed by the caller) is then set to 1
 * and that top is not reported; the caller must not use the triplets of a call that set it. A non-empty own range must lie inside the
 * band; bad arguments return GENIE_ERR_ARG before any launch. */
int genie_band_peaks_count(const float* band, int rows, int64_t width, int64_t stride, int64_t b_lo, int64_t o_lo, int64_t o_hi,
                           int64_t n_cols, float threshold, int32_t* counts, int32_t* flag, void* stream);
int genie_band_peaks_fill(const float* band, int rows, int64_t width, int64_t stride, int64_t b_lo, int64_t o_lo, int64_t o_hi,
                          int64_t n_cols, float threshold, const int64_t* offsets, int32_t* out_row, int32_t* out_col, float* out_val,
                          int32_t* flag, void* stream);

/* Peak candidates of a STREAM of column blocks (the closed columns of the online day loop, genie_amd/postproc.py::StreamPeaks,
 * OnlineDetector): block [rows, width] fp32 with row stride `stride` (elements; columns contiguous) holds the global columns
 * [c0, c0 + width) of an axis of n_cols columns; the blocks of a stream arrive in order and without gaps, the first with c0 = 0. Over
 * the whole stream the calls write exactly the mode-1 peaks of the row selection above on the full matrix -- local maxima >= threshold,
 * flat tops at their midpoint (start + end) / 2, never a run that holds global column 0 or n_cols - 1 -- as triplets (row, GLOBAL column,
 * value), row-major within a call, a row's columns ascending within a call and from call to call.
 * The carry: genie_stream_peaks_carry_bytes(rows) bytes per buffer (16 per row, 16-byte aligned), two buffers that the caller swaps
 * after every COUNT call that launched. Per row it holds the value of column c0 - 1, the global column where the run that holds it
 * began, and whether the value before that run was lower. carry_in is not read when c0 = 0 (it must still be non-null).
 * A call decides every run whose end it knows: the runs that end inside the block with their successor in the block, and the carried run
 * when the block's first value differs from the carried one -- emitted first in its row, at a midpoint that may lie several blocks
 * back. A run that reaches the block's last column is deferred through the carry (if that column is n_cols - 1 it is no peak). There is no
 * flag and no fallback: every flat top is decided exactly.
 * Two passes: genie_stream_peaks_count reads carry_in and writes carry_out, counts [rows] and bound [1]; the caller turns the counts
 * into exclusive int64 offsets [rows]; genie_stream_peaks_fill reads the SAME carry_in and writes the triplets at offsets[row] + rank
 * (no atomics on the output; it may be skipped when the total is 0).
 * bound (int64 [1], written by every COUNT call that launches): no triplet of any LATER call of the stream has a column below it. It is
 * c0 + width, lowered to (start + c0 + width - 1) / 2 for every row whose run is still open after the block, reaches the threshold,
 * rose and does not hold column 0 (the smallest midpoint that run can still get); n_cols after the block that ends the axis.
 * rows = 0 or width = 0: no launch, the carry and the bound stay as they are. Bad arguments (a negative size, n_cols >= 2^31, c0 < 0,
 * c0 + width > n_cols, width > 1 with stride < width, a null pointer with rows and width positive) return GENIE_ERR_ARG before any
 * launch. */
size_t genie_stream_peaks_carry_bytes(int rows);
int genie_stream_peaks_count(const float* block, int rows, int64_t width, int64_t stride, int64_t c0, int64_t n_cols, float threshold,
                             const void* carry_in, void* carry_out, int32_t* counts, int64_t* bound, void* stream);
int genie_stream_peaks_fill(const float* block, int rows, int64_t width, int64_t stride, int64_t c0, int64_t n_cols, float threshold,
                            const void* carry_in, const int64_t* offsets, int32_t* out_row, int32_t* out_col, float* out_val,
                            void* stream);

/* Column occupancy of a stream's candidates (genie_amd/postproc.py::OnlineDetector): ring[cols[i] mod W] += 1 for every i < n, with
 * integer atomics (the counts do not depend on the schedule), one thread per candidate. cols [n] int32, the non-negative global columns
 * genie_stream_peaks_fill wrote (the slot is taken on the unsigned value: always inside the ring); ring [W] int32, which the caller
 * zeroes once and where it clears the slots of the columns it releases. The call ACCUMULATES: the caller keeps the live columns within
 * one span of W, so that a slot stands for one column. n = 0: no launch. Bad arguments (n < 0 or >= 2^31, W < 1 or >= 2^31, a null
 * pointer with n > 0) return GENIE_ERR_ARG before any launch. */
int genie_col_counts(const int32_t* cols, int64_t n, int32_t* ring, int64_t W, void* stream);

/* The time-pointer tables of the association heads on the device (`assemble_time_pointers_for_stations`, utils.py:602-622, called at
 * train_GENIE_model.py:1364 and process_continuous_days.py:620; genie_amd/graph.py::time_pointers is the host statement): for every
 * station i and every time step t of dt_partition, the k candidates of station i that are smallest under the key
 *   ( |(double)trv - t| , product-node id ),   nearest first, equal distances to the lower id,
 * the subtraction and the absolute value in fp64 on the fp32 travel time widened exactly. The key is a total order, so the tables are
 * unique: equal to the reference's stable argsort of |trv - t| over all source nodes, bit for bit, ties included.
 *   trv [n_prod, 2] fp32: P / S travel time of every product node, in product-node order (`tlatent` of set_adjacencies); must be finite.
 *   sta_of_prod NULL: the Cartesian product, node p = g * n_sta + i (n_prod a multiple of n_sta); the candidates of station i are its
 *     G = n_prod / n_sta nodes. The caller passes k <= G (the reference clips k to G).
 *   sta_of_prod [n_prod] int32: an irregular product graph (`use_subgraph`), the station of every product node; the candidates of station
 *     i are the nodes listing it. A station with n < k candidates gets rank j filled with rank j mod n (this package's own rule: the
 *     reference has no fixture for irregular tables); a station with none gets zeros and is counted in status[0].
 *   dt_partition [n_t] fp64 on the device, ascending; 1 <= k <= 32.
 *   edges_p / edges_s: int32 [n_sta * n_t * k] each, laid out [station][time step][k] (what LocalSliceLgCollapse indexes, module.py:635-637,
 *     and genie_lslc_fwd takes), both written by the one call.
 *   status [2] int32 on the device, written by the call: [0] = stations without a candidate, [1] = 1 when a travel time was inf / NaN
 *     (such entries are never listed). Nothing is read back here; the caller reads status when it wants the verdict.
 *   scratch: genie_time_pointers_scratch_bytes(n_prod, n_sta, n_t) bytes on the device, 16-byte aligned, contents irrelevant before and
 *     after (16 bytes per product node plus the bin tables; 0 when the sizes are out of contract).
 * Every size lives in global memory: no limit on the nodes of a station. The order in which candidates meet inside the call depends on
 * scheduling, the tables do not: two calls write the same bits. Vector stores and vector atomics only. Bad arguments (k < 1, k > 32,
 * n_t < 2, n_prod < 1 or >= 2^31, n_sta < 1, n_prod not a multiple of n_sta in the Cartesian form, n_sta x n_t beyond one launch, a null
 * pointer, misaligned scratch) return GENIE_ERR_ARG before any launch. */
size_t genie_time_pointers_scratch_bytes(int64_t n_prod, int n_sta, int n_t);
int genie_time_pointers(const float* trv, int64_t n_prod, int n_sta, const int32_t* sta_of_prod, const double* dt_partition, int n_t, int k,
                        void* scratch, int32_t* edges_p, int32_t* edges_s, int32_t* status, void* stream);

/* The same tables of a source-node-sharded model (Cartesian form), built from each rank's OWN travel-time rows: candidates per rank, one
 * all-gather of the fixed-size key blocks by the caller, merge on every rank. Both kernels rank with genie_time_pointers' key and its
 * wave-wide insertion, so the tables are those of genie_time_pointers over the whole product graph, bit for bit.
 * genie_time_pointers_candidates: trv_own [n_prod_own, 2] = the rows of the rank's owned source nodes in its local node order (local
 *   row l * n_sta + i), node_global int32 [n_prod_own / n_sta]: local source node -> global one (global product node = g * n_sta + i,
 *   which must stay below 2^31). cand: int64 [2][n_sta][n_t][k][2], 16-byte aligned: per (phase, station, time step) the rank's
 *   min(k, n_own) smallest keys, ascending, each as (the bits of the float64 distance, the GLOBAL product-node id); the remaining
 *   slots hold the key (max double, 2^31 - 1), which sorts after every candidate -- a rank that owns fewer than k nodes does not cycle.
 *   scratch: genie_time_pointers_scratch_bytes(n_prod_own, n_sta, n_t); status [2] as genie_time_pointers.
 * genie_time_pointers_merge: cand int64 [world][2][n_sta][n_t][k][2] = every rank's block, in any rank order -> the k_out <= k smallest
 *   keys per entry, nearest first, as int32 ids in edges_p / edges_s [n_sta * n_t * k_out]. status [1] int32: 1 when an entry has
 *   fewer than k_out real keys (the blocks do not cover the station). The caller passes k_out = min(k, number of source nodes). */
int genie_time_pointers_candidates(const float* trv_own, int64_t n_prod_own, int n_sta, const int32_t* node_global, const double* dt_partition,
                                   int n_t, int k, void* scratch, int64_t* cand, int32_t* status, void* stream);
int genie_time_pointers_merge(const int64_t* cand, int world, int n_sta, int n_t, int k, int k_out, int32_t* edges_p, int32_t* edges_s,
                              int32_t* status, void* stream);

/* Stacking of window read-outs into Out_2 (the apply loop's accumulation, process_continuous_days.py:797-805), one launch per flush:
 *   for k in 0..n_windows-1 (window order), for j in 0..n_offsets-1 (offset order):
 *       c = cols[k][j];  if c < 0: skip;   out[q, c] += x[k, q, j] * scale   for every query q
 * x [n_windows, n_query, n_offsets] fp32 (the read-out of genie_tail_batched, or of one window: n_windows = 1); cols [n_windows, n_offsets]
 * int32 ON THE DEVICE (-1 drops an offset: the last offset of step_size 'half', or all but the last occurrence of a column one window
 * lists twice); out [n_query, n_cols] fp32, addressed with 64-bit element offsets; [c_min, c_max] = a column range that contains every
 * entry >= 0 of cols: an entry outside it is ignored, nothing outside out[:, c_min..c_max] is read or written. 1 <= n_windows <= 16,
 * 1 <= n_offsets <= 64, 1 <= n_cols < 2^31. No atomics: one thread owns one (q, c) and adds its contributions in (k, j) order, the product
 * rounded to fp32 before the add, so the result is reproducible and carries the bits of `out.index_add_(1, cols_k, x_k * scale)` issued
 * window by window. `scale`: the caller's fp32 factor (torch divides a tensor by a host scalar d as `x * (1.0f / (float)d)`; pass that
 * reciprocal to match it). This is genie_stack_windows_legs with the one leg x: the same kernel and the same launch. A null x or out
 * passes only with n_query == 0. Bad arguments return GENIE_ERR_ARG before any launch. */
int genie_stack_windows(const float* x, const int32_t* cols, int n_windows, int64_t n_query, int n_offsets, float scale, float* out,
                        int64_t n_cols, int64_t c_min, int64_t c_max, void* stream);

/* The same stacking over the source grids ("legs") of a day (process_continuous_days.py:761-810: every window runs on every grid and all
 * of them add into the one Out_2), one launch per flush of all legs:
 *   for k in 0..n_windows-1, for j in 0..n_offsets-1, for l in 0..n_legs-1 (innermost):
 *       c = cols[k][j];  if c < 0: skip;   out[q, c] += x_legs[l][k, q, j] * scale   for every query q
 * A row of cols that lists no column twice (apply.window_cols_table makes only such rows) feeds an element of out at most once per window,
 * so the order is exactly `for window: for leg: out.index_add_(1, cols_k, x_l[k] * scale)`; a row that does list a column twice adds
 * twice, in (k, j, l) order. x_legs: HOST array of n_legs device pointers, each to fp32 [n_windows, n_query, n_offsets] (64-bit element
 * offsets); the pointers travel in the kernel arguments, so the call copies nothing and never waits. 1 <= n_legs <= 32; cols, out,
 * [c_min, c_max], scale and the ranges of n_windows, n_offsets, n_cols as in genie_stack_windows, which is the n_legs = 1 case of this
 * entry (one kernel serves both). No atomics, the product rounded before the add; an element no entry lists is not written. Bad
 * arguments (a null table, a null pointer in it, n_legs outside 1..32, any range error of genie_stack_windows) return GENIE_ERR_ARG
 * before any launch; n_legs and the pointer table are checked first, then the ranges, then cols and out. */
int genie_stack_windows_legs(const float* const* x_legs, int n_legs, const int32_t* cols, int n_windows, int64_t n_query, int n_offsets,
                             float scale, float* out, int64_t n_cols, int64_t c_min, int64_t c_max, void* stream);

/* The same stacking into a RING of open columns (the online day loop, apply.OnlineDay, whose Out_2 never exists as a whole): ring
 * [n_query, ring_cols] fp32 and column c of the day lives in slot c % ring_cols,
 *   for k, for j, for l (innermost):  c = cols[k][j];  if c < 0: skip;   ring[q, c % ring_cols] += x_legs[l][k, q, j] * scale
 * cols holds ABSOLUTE columns of the day (0 <= c < 2^31), [c_min, c_max] contains every entry >= 0 as in genie_stack_windows, and the
 * call is refused with GENIE_ERR_ARG, before any launch and writing nothing, when c_max - c_min >= ring_cols: two columns of one call
 * never share a slot. That a slot holds nothing of an older column is the caller's business (genie_ring_close frees slots). One kernel
 * serves this entry and genie_stack_windows_legs, so a column's running sum (windows in ascending order, legs in order, the product
 * rounded before the add) carries the same bits in the ring as in a dense Out_2. Every other argument, range and error as there. */
int genie_stack_windows_ring(const float* const* x_legs, int n_legs, const int32_t* cols, int n_windows, int64_t n_query, int n_offsets,
                             float scale, float* ring, int64_t ring_cols, int64_t c_min, int64_t c_max, void* stream);

/* Columns [c_lo, c_hi) leave the ring: out[q, j] = ring[q, (c_lo + j) % ring_cols] for j < c_hi - c_lo, out dense [n_query, c_hi - c_lo]
 * fp32, and those slots are set to zero -- one pass, every slot read and zeroed by the one thread that owns it. c_hi - c_lo <= ring_cols
 * (a range may wrap the ring's end), 0 <= c_lo <= c_hi <= 2^31, n_query < 2^31; an empty range or n_query == 0 returns GENIE_OK without
 * a launch. Bad arguments return GENIE_ERR_ARG before any launch. */
int genie_ring_close(float* ring, int64_t n_query, int64_t ring_cols, int64_t c_lo, int64_t c_hi, float* out, void* stream);

/* A checkpoint of the ring's open columns (apply.OnlineDay.state_dict): genie_ring_close without the zeroing,
 *   out[q, j] = ring[q, (c_lo + j) % ring_cols]   for j < c_hi - c_lo,  out dense [n_query, c_hi - c_lo] fp32,
 * and the ring is only read. One launch, one thread per element; arguments, ranges and errors as genie_ring_close. */
int genie_ring_save(const float* ring, int64_t n_query, int64_t ring_cols, int64_t c_lo, int64_t c_hi, float* out, void* stream);

/* The inverse store (apply.OnlineDay.load_state_dict): ring[q, (c_lo + j) % ring_cols] = block[q, j] for j < c_hi - c_lo, block dense
 * [n_query, c_hi - c_lo] fp32. ring_cols is this ring's own and need not be that of the ring the block was saved from, only
 * >= c_hi - c_lo; exactly those slots are written (each by the one thread that owns it) and no others. One launch; arguments, ranges and
 * errors as genie_ring_close. */
int genie_ring_load(float* ring, int64_t n_query, int64_t ring_cols, int64_t c_lo, int64_t c_hi, const float* block, void* stream);

/* Merge by rank of two time-sorted runs of picks (the growable pick store of the online day loop, apply.PickStore): the resident run a
 * (n_a picks) and a chunk b (n_b picks), each given as four arrays on the device -- t fp64 ascending, sta int32, phase int32, index int64
 * -- into the four output arrays of n_a + n_b elements, which must not overlap the inputs:
 *   a[i] lands at i + #{j: t_b[j] < t_a[i]},     b[j] lands at j + #{i: t_a[i] <= t_b[j]}
 * the stable merge in which a resident pick precedes a chunk pick of the same time, i.e. a stable sort by time of a followed by b. One
 * thread per element and a binary search in the other run; every output position is written exactly once, no atomics, and the result
 * does not depend on scheduling. A run that is not ascending gives an unspecified permutation, never an access outside the arrays.
 * n_a + n_b == 0 returns GENIE_OK without a launch; an empty run may pass null pointers. Bad arguments (a negative count, a null
 * pointer of a non-empty run or of the output) return GENIE_ERR_ARG before any launch. */
int genie_picks_merge(const double* t_a, const int32_t* sta_a, const int32_t* phase_a, const int64_t* index_a, int64_t n_a, const double* t_b,
                      const int32_t* sta_b, const int32_t* phase_b, const int64_t* index_b, int64_t n_b, double* t_out, int32_t* sta_out,
                      int32_t* phase_out, int64_t* index_out, void* stream);

/* The pick lists of one window (apply.ResidentPicks.pick_inputs, extract_pick_inputs_from_data of the reference) in one launch: the n
 * picks of a contiguous range of the time-sorted store (t fp64, sta int32 in [0, n_sta), phase int32, index int64, on the device), cut by
 * the ball query when ball != 0 -- kept where fabs(t - centre) <= radius in fp64 -- and stable-sorted by station (a counting sort: within
 * a station the picks keep the order of the range). Written, for the m kept picks in that order: tp_out = t - t0 (fp64), ip_out = station
 * (int64), ph_out = phase (fp64), idx_out = index (int64), each with room for n elements (the elements from m on are not touched), and
 * count_out[0] = m (int64, on the device). One workgroup of 256 threads; the station histogram and its exclusive scan live in LDS, so
 * n_sta <= genie_pick_lists_max_sta() (8192): a larger station set returns GENIE_ERR_ARG and the caller sorts by other means. Every
 * output element is written once with a vector store, nothing is atomic in global memory, and the result does not depend on
 * scheduling. A pick whose station lies outside [0, n_sta) is left out and never used as an index. n == 0 writes count_out[0] = 0 and
 * may pass null arrays. Bad arguments (n outside [0, 2^31), n_sta outside the table, a null pointer, a ball that is not finite) return
 * GENIE_ERR_ARG before any launch. */
int genie_pick_lists_max_sta(void);
int genie_pick_lists(const double* t, const int32_t* sta, const int32_t* phase, const int64_t* index, int64_t n, int n_sta, double t0,
                     int ball, double centre, double radius, double* tp_out, int64_t* ip_out, double* ph_out, int64_t* idx_out,
                     int64_t* count_out, void* stream);

/* Selection of the refined source out of the grid legs' query read-outs (the refine pass, process_continuous_days.py:972-978), one call
 * per candidate source instead of a chain of full passes over [n_query, n_t]:
 *   acc[q, t] = fp32 sum over l = 0..n_used-1, in that order and starting from 0.0f, of x[l][q, t] / n_scale, computed as torch computes
 *               `acc += x_l / n_scale` for a host scalar n_scale: x * (1.0f / n_scale), the product rounded before the add;
 *   rows with keep[q] == 0 count as -inf (keep NULL: every row is kept);
 *   ip = the first row whose row maximum equals the global maximum, it = the first column of that row holding its maximum,
 *   out[0..3] = (ip, it, acc[ip, it], any_kept) as fp64; any_kept = 1 when a kept row exists, else 0 and out = (0, 0, -inf, 0).
 * x: HOST array of n_used device pointers, each to fp32 [n_query, n_t] (row-major, 64-bit element offsets); the pointers travel in the
 * kernel arguments, so the call copies nothing and never waits. n_used = the legs that produced a window, 0 <= n_used <= 32 (0: acc is
 * all zero, the first kept row and column 0 win); n_scale = the number of legs of the average, finite and > 0. keep [n_query] uint8 on
 * the device. scratch: genie_refine_select_scratch_bytes() bytes on the device, 16-byte aligned, contents irrelevant before and after.
 * Equal to the nested argmax bit for bit, ties included; no atomics, the result does not depend on scheduling. NaN inputs are out of
 * scope (the read-outs are finite sigmoid outputs; the library is built without NaN semantics). n_query >= 0, n_t >= 1. Bad arguments
 * (a null pointer, a negative count, n_t < 1, n_used > 32, n_scale <= 0) return GENIE_ERR_ARG before any launch. */
size_t genie_refine_select_scratch_bytes(void);
int genie_refine_select(const float* const* x, int n_used, int64_t n_query, int n_t, const uint8_t* keep, float n_scale, void* scratch,
                        double* out, void* stream);

/* genie_refine_select for a batch of sources in one launch pair: row b of out [n_batch, 4] carries the bits genie_refine_select gives for
 * source b alone. x: DEVICE table [n_batch, n_legs] of device pointers, entry (b, l) = leg l's read-out fp32 [n_query, n_t] of source b,
 * or NULL where that leg produced no window for the source: source b's sum runs over its non-null legs in leg order (the single form's
 * n_used pointers); a row of NULLs is an all-zero acc. keep [n_batch, n_query] uint8 on the device or NULL; scratch: n_batch *
 * genie_refine_select_scratch_bytes() bytes, 16-byte aligned. 1 <= n_batch <= 65535, 0 <= n_legs <= 32; otherwise as the single form. */
int genie_refine_select_batch(const float* const* x, int n_batch, int n_legs, int64_t n_query, int n_t, const uint8_t* keep, float n_scale,
                              void* scratch, double* out, void* stream);

/* The query cloud of one candidate source of the refine pass (process_continuous_days.py:929, :934), drawn on the device by a keyed
 * counter-based generator, one launch per source and nothing copied from the host:
 *   r   = np.random.Generator(np.random.Philox(key=[key0, key1], counter=[0, source, 0, 0])).random((n_query, 3))     as bits: flat
 *         element j of the row-major [n_query, 3] array is word j % 4 of Philox4x64-10 block j / 4, whose counter is (j / 4 + 1, source,
 *         0, 0) (numpy increments counter word 0 before it generates), made a double as (u >> 11) * 2^-53;
 *   xc[q, a] = s[a] + (r[q, a] * rng[a] + mn[a])   in fp64, every operation rounded on its own (no fused multiply-add): the bits of the
 *         numpy / torch statement `src + (r * X_offset_range + X_offset_min)`; s = (sx, sy, sz) the source's Cartesian position,
 *         rng = (rx, ry, rz) = X_offset_range, mn = (mx, my, mz) = X_offset_min;
 *   xq[q, a] = (float)xc[q, a], round to nearest even (`xc.astype(float32)`, `Xc.float()`).
 * The draw depends on (key0, key1, source, element) alone: any rank, any launch and any split of the sources over GPUs gives the same
 * cloud for a source, and a source nobody asks for costs nothing. Everything small travels by value in the kernel arguments, so the call
 * copies nothing and never waits. r [n_query, 3] fp64 or NULL (the draw is not stored), xc [n_query, 3] fp64, xq [n_query, 3] fp32, all on
 * the device, row-major, 16-byte aligned, addressed with 64-bit element offsets. No atomics, no scratch; two calls with the same
 * arguments write the same bits. Non-finite or absurd offsets are the caller's: they propagate as IEEE arithmetic has them.
 * n_query == 0 returns GENIE_OK without a launch and touches nothing. Bad arguments (n_query < 0, or with n_query > 0 a null xc or xq, a
 * pointer that is not 16-byte aligned, n_query > 2^60) return GENIE_ERR_ARG before any launch. */
int genie_refine_cloud(uint64_t key0, uint64_t key1, uint64_t source, int64_t n_query, double sx, double sy, double sz, double rx, double ry,
                       double rz, double mx, double my, double mz, double* r, double* xc, float* xq, void* stream);

/* genie_refine_cloud for the sources source0 .. source0 + n_batch - 1 in one launch: row block b of xc [n_batch, n_query, 3] fp64 and xq
 * [n_batch, n_query, 3] fp32 carries the bits of genie_refine_cloud(key0, key1, source0 + b, n_query, src_cart[b], ...). src_cart
 * [n_batch, 3] fp64 ON THE DEVICE (8-byte aligned): the sources' Cartesian positions; the ranges and minima are the batch's. xc and xq
 * 16-byte aligned. The draw itself is not stored. 1 <= n_batch <= 65535; n_query == 0 returns GENIE_OK without a launch. */
int genie_refine_cloud_batch(uint64_t key0, uint64_t key1, uint64_t source0, int n_batch, int64_t n_query, const double* src_cart, double rx,
                             double ry, double rz, double mx, double my, double mz, double* xc, float* xq, void* stream);

/* The optimizer step of a training batch in one launch: the ranks' gradient parts summed in rank order, then torch.optim.Adam's update
 * (defaults: no weight decay, no amsgrad, not maximize; train_GENIE_model.py:1383, :1861) on flat arrays. Needs no context. Per element j:
 *   g = 0.0f;  for r = 0 .. n_parts-1:  g = g + grad_parts[r * part_stride + j]      fp32, in that order, never fused or reassociated:
 *       the bits of `g = zeros; g += part_r` part by part (one part: g is that part as a value);
 *   m = fma(g - m, 1 - beta1, m);   v = fma((1 - beta2) * g, g, beta2 * v);
 *   p = p + (-(lr / (1 - beta1^step)) * m) / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * in fp32, operation by operation as torch's single-tensor Adam rounds it on the CPU (lerp_ and addcmul_ end in one fused multiply-add
 * each, written out here; everything else is rounded on its own: mul_, sqrt / div / add_, addcdiv_); square root and division are
 * correctly rounded. step >= 1 is the step being taken; the scalars 1 - beta1, 1 - beta2,
 * lr / (1 - beta1^step) and sqrt(1 - beta2^step) are formed here in double and rounded to fp32 once. An element with g = m = v = 0
 * keeps the bits of p, m and v (a parameter that never gets a gradient rides along as zeros). param, exp_avg (m), exp_avg_sq (v) [n]
 * fp32 on the device, updated in place; grad_parts: n_parts arrays of n floats, part r at grad_parts + r * part_stride (part_stride in
 * floats, ignored for one part); grad_out [n] or NULL receives g and must not overlap the parts. 16-byte accesses are used where the
 * pointers (and part_stride) are multiples of 16 bytes, 4-byte ones otherwise: any layout gives the same bits. 64-bit offsets, no
 * atomics, no scratch; two calls with the same arguments and state write the same bits. n == 0 returns GENIE_OK without a launch. Bad
 * arguments (n < 0, n_parts < 1 or > 32, step < 1, with n > 0 a null param / exp_avg / exp_avg_sq / grad_parts, a pointer that is not
 * 4-byte aligned, beta outside [0, 1), negative eps, non-finite lr / eps) return GENIE_ERR_ARG before any launch and touch nothing. */
int genie_adam_step(float* param, float* exp_avg, float* exp_avg_sq, int64_t n, const float* grad_parts, int n_parts, int64_t part_stride,
                    float* grad_out, double lr, double beta1, double beta2, double eps, int64_t step, void* stream);

/* Debug/parity access to intermediates kept in the workspace (which: 0 = c [P,30], 1 = wu [P,15], 2 = wv [P,15]);
 * copies de-padded rows into `out` (async). */
int genie_ws_export(genie_ctx* ctx, int which, void* ws, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GENIE_HIP_H */
