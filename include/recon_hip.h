/*
 * recon_hip.h — C ABI of librecon_hip.so: MI355X (gfx950) kernels for RECON's graph-context
 * aggregation hot path.
 *
 * The reference (ansonb/RECON) is pure Python: it has no FFI of its own.  Its "plugin boundary"
 * for this path is the Python class surface of GAT/layers.py and models/layers.py; the drop-in
 * modules in recon_amd/ keep that surface and bind the entry points below with ctypes
 * (INTEGRATION.md shows the stub).  Each entry point names the reference lines it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless marked "host";
 *   - the caller owns every buffer (inputs, outputs, workspaces); the library allocates nothing
 *     and keeps no mutable global state;
 *   - every call only ENQUEUES work on `stream` (a hipStream_t); it never synchronises;
 *   - return value: 0 = RECON_OK, negative = error (recon_error_string()); no C++ exception
 *     crosses this boundary;
 *   - float tensors are fp32, row-major, contiguous unless a leading dimension is given;
 *     indices handed over by the reference API are int64 (torch.LongTensor), internal index
 *     arrays are int32.
 */
#ifndef RECON_HIP_H
#define RECON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RECON_ABI_VERSION 2

enum {
    RECON_OK = 0,
    RECON_ERR_INVALID = -1,     /* null pointer / negative size / inconsistent dims   */
    RECON_ERR_UNSUPPORTED = -2, /* shape outside what the kernels are instantiated for */
    RECON_ERR_LAUNCH = -3,      /* hipGetLastError() != hipSuccess after a launch      */
    RECON_ERR_WORKSPACE = -4    /* workspace smaller than recon_*_workspace_bytes()    */
};

typedef void* recon_stream_t; /* hipStream_t */

int recon_version(void);
const char* recon_error_string(int code);

/* Run-time switches (recon_amd/csrc/config.hip): one table, filled from the environment variables of the same names (RECON_GEMM_CFG,
 * RECON_PROP_FWD ... — INTEGRATION.md lists them) the first time the library needs one; every switch chooses between kernels that
 * compute the same result.  recon_config_set overrides one entry (value NULL: unset), recon_config_get returns the current value or NULL.
 * Call them between launches, from the launching thread.  The reference has no counterpart (its only switch is the module-level CUDA flag,
 * GAT/layers.py:10). */
/* Optional NaN word of a device (int32, device memory, zeroed by the caller; NULL: off): the attention kernels store 1 into it when a row sum
 * of attention weights comes out NaN or infinite — the condition behind the reference's three `assert not torch.isnan(...)` per layer call
 * (GAT/layers.py:147, :167, :172), without their three host round trips: nothing waits for the word, the caller reads it when it likes. */
int recon_set_nan_flag(int32_t device, int32_t* flag);
int recon_config_set(const char* name, const char* value);
const char* recon_config_get(const char* name);

/* --------------------------------------------------------------------------------------------
 * K3  graph preparation: COO edge list -> destination-CSR + source-CSC views.
 * Replaces the implicit coalesce/sort inside torch.sparse.sum at GAT/layers.py:56-58 (and the
 * edge concatenation at GAT/layers.py:124-127, done by the caller on the index tensors).
 * Stable: edges of one destination keep their original relative order; duplicates are kept.
 * ------------------------------------------------------------------------------------------*/
typedef struct {
    int32_t N;                  /* nodes                                                     */
    int32_t E;                  /* edges (1-hop + n-hop)                                     */
    int32_t* rowptr_dst;        /* [N+1] CSR over destinations (edge[0,:], the segment id)   */
    int32_t* eid;               /* [E]   CSR slot -> original edge column                    */
    int32_t* src;               /* [E]   source node (edge[1,:]) of each CSR slot            */
    int32_t* dst;               /* [E]   destination node of each CSR slot                   */
    int32_t* rowptr_src;        /* [N+1] CSC over sources; NULL at build: destination CSR only (src, slot_by_src unused) */
    int32_t* slot_by_src;       /* [E]   CSC position -> CSR slot                            */
    /* Hub rows (optional; all zero = every destination row is walked by one wave, whatever its length).  The aggregate-then-
     * project edge kernels give one wavefront to one destination node; a node with hundreds of in-edges (power-law graphs)
     * is then one long serial chain.  With these tables a row of more than hub_chunk slots is cut into pieces of at most
     * hub_chunk slots, each walked by its own wavefront, and summed in table order by a second small launch: results do not
     * depend on scheduling.  Filled by recon_graph_hubs_count() + recon_graph_hubs_fill().                              */
    int32_t hub_chunk;          /* slots per piece (RECON_HUB_CHUNK), 0: no splitting                                    */
    int32_t n_hub;              /* destination nodes with more than hub_chunk slots                                      */
    int32_t n_piece;            /* their pieces                                                                          */
    int32_t* hub_node;          /* [n_hub]     node id, ascending                                                        */
    int32_t* hub_ptr;           /* [n_hub + 1] first piece of each hub                                                   */
    int32_t* piece;             /* [n_piece][4] (node, first slot, end slot, hub ordinal), 16-byte aligned               */
    /* the same for the source-side walk of the backward (CSC rows: a node that is the neighbour in many edges) */
    int32_t n_hub_src, n_piece_src;
    int32_t* hub_node_src;      /* [n_hub_src]                                                                           */
    int32_t* hub_ptr_src;       /* [n_hub_src + 1]                                                                       */
    int32_t* piece_src;         /* [n_piece_src][4] (node, first CSC position, end position, hub ordinal)                */
    float* hub_ws;              /* scratch of the piece partial sums, reused by every call on this graph (calls on one graph
                                   are stream ordered): at least recon_graph_hub_ws_floats() floats for the widest layer   */
    int64_t hub_ws_floats;
    /* Row compaction (optional; n_rows = 0: every node is a row).  A knowledge-graph batch (GAT/main.py:478-516) aggregates into the
     * batch's ~128 entities of a 14 541-entity table: all other destination rows are empty, their layer output is exactly 0
     * (GAT/layers.py:152-158: 0 / 1e-12, elu(0) = 0) and so is everything they contribute backward.  With these tables the
     * aggregate-then-project kernels run their node-parallel stages (V, the three GEMMs, g_V, the destination walk of the backward)
     * over the n_rows rows WITH edges; `out` / `grad_out` of recon_gat_atp_args then hold n_rows rows / are read through row_node.
     * The hub tables of the destination side name ROWS when these are set.  Filled by recon_graph_rows_compact().            */
    int32_t n_rows;             /* destination nodes with at least one in-edge                                              */
    int32_t* row_node;          /* [n_rows]     node id of each row, ascending                                              */
    int32_t* rowptr_rows;       /* [n_rows + 1] first CSR slot of each row (rowptr_dst without the empty rows)              */
    int32_t* node_row;          /* [N]          row of each node, -1: none                                                  */
} recon_graph;

#define RECON_HUB_CHUNK 64

size_t recon_graph_workspace_bytes(int32_t N, int32_t E);
/* Hub tables of a built graph.  count: one pass over rowptr_dst and one over rowptr_src, synchronises the stream and returns the
 * table sizes counts[4] = (n_hub, n_piece, n_hub_src, n_piece_src); all zero: nothing to do.  fill: the caller has set hub_chunk
 * and the four sizes to what count returned and the six table pointers to device arrays of those sizes (a side without hubs may
 * stay NULL).  hub_ws may be set (or grown) at any time before a layer call. */
int recon_graph_hubs_count(const recon_graph* g, int32_t chunk, void* workspace /* device, 16 bytes */, int32_t* counts /* host [4] */,
                           recon_stream_t stream);
int recon_graph_hubs_fill(const recon_graph* g, recon_stream_t stream);
/* The same two calls with the build's range check riding along: recon_graph_build_checked sets *bad (device int32, zero on entry) when an
 * id lies outside [0, N) — the tables are then garbage and must not be used; recon_graph_hubs_count_checked copies the flag to *bad_host in
 * the round trip it makes anyway (the reference fails on such input with an index error: GAT/layers.py:56, torch.sparse_coo_tensor). */
int recon_graph_build_checked(const int64_t* edge_dst, const int64_t* edge_src, recon_graph* g, void* workspace, size_t workspace_bytes,
                              int32_t* bad, recon_stream_t stream);
int recon_graph_hubs_count_checked(const recon_graph* g, int32_t chunk, void* workspace, int32_t* counts, const int32_t* bad, int32_t* bad_host,
                                   recon_stream_t stream);
/* Build + hub-table sizes in one chain: recon_graph_build_counted is recon_graph_build_checked whose last launch also counts, for rows
 * of more than `chunk` slots, the four sizes recon_graph_hubs_count would return (they stay in the workspace: one launch less per build —
 * a build is a chain of small dependent launches); recon_graph_hubs_read copies them (and the range-check flag, which that last launch
 * stores behind the sizes: `bad` given to recon_graph_hubs_read only says that *bad_host is wanted — it must be the build's) to the host in
 * one copy, with the one synchronisation of the pair.  The graph needs both views (rowptr_src set); `workspace` is the build's. */
int recon_graph_build_counted(const int64_t* edge_dst, const int64_t* edge_src, recon_graph* g, void* workspace, size_t workspace_bytes,
                              int32_t* bad, int32_t chunk, recon_stream_t stream);
int recon_graph_hubs_read(const recon_graph* g, void* workspace, int32_t* counts /* host [4] */, const int32_t* bad, int32_t* bad_host,
                          recon_stream_t stream);
/* floats of hub_ws one KB-GAT layer call (forward or backward) on this graph needs */
size_t recon_graph_hub_ws_floats(const recon_graph* g, int32_t F, int32_t R, int32_t H);
/* recon_graph_hubs_read that also returns the number of destination rows with edges (*live_rows; counted by recon_graph_build_counted's
 * last launch): the caller decides on row compaction from it.  recon_graph_rows_compact: g->n_rows = that count, row_node / rowptr_rows /
 * node_row point to device arrays of n_rows / n_rows + 1 / N int32; one launch; call it BEFORE recon_graph_hubs_fill (whose destination
 * tables are then built over the rows). */
int recon_graph_counts_read(const recon_graph* g, void* workspace, int32_t* counts /* host [4] */, int32_t* live_rows /* host, may be NULL */,
                            const int32_t* bad, int32_t* bad_host, recon_stream_t stream);
int recon_graph_rows_compact(const recon_graph* g, recon_stream_t stream);
/* out[n, :] = rows[node_row[n], :] or 0 (node_row[n] < 0): the layer output of a row-compacted graph back in node order. */
int recon_rows_expand(const float* rows, int32_t ld_rows, const int32_t* node_row, int32_t N, int32_t width, float* out, int32_t ld_out,
                      recon_stream_t stream);

/* edge_dst / edge_src: the two rows of the reference's int64 [2,E] edge tensor (row 0 =
 * aggregation target, row 1 = neighbour; GAT/create_batch.py:429-433).  Returns RECON_ERR_INVALID
 * if N or E overflow int32.  Node ids outside [0,N) are undefined behaviour (as in the reference). */
int recon_graph_build(const int64_t* edge_dst, const int64_t* edge_src, recon_graph* g,
                      void* workspace, size_t workspace_bytes, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * G1-G3  SpecialSpmmFinal: out[r,:] = sum_{e: edge[0,e]==r} edge_w[e,:]   (GAT/layers.py:54-64)
 *        backward: grad_edge_w[e,:] = grad_out[edge[0,e],:]               (GAT/layers.py:67-79)
 * ------------------------------------------------------------------------------------------*/
size_t recon_spmm_rowsum_workspace_floats(int32_t E, int32_t out_features);
int recon_spmm_rowsum_fwd(const recon_graph* g, const float* edge_w /*[E,out_features]*/,
                          int32_t out_features, float* out /*[N,out_features]*/,
                          float* workspace /* recon_spmm_rowsum_workspace_floats() floats */, recon_stream_t stream);
/* the same with `row_mod` > 0: slot e reads row (eid[e] % row_mod) of edge_w — several keys share one value row (the gradient of
 * table[i0] + table[i1]: keys (i0 | i1), E value rows) */
int recon_spmm_rowsum_mod_fwd(const recon_graph* g, const float* edge_w, int32_t out_features, int32_t row_mod, float* out,
                              float* workspace, recon_stream_t stream);
int recon_spmm_rowsum_bwd(const int64_t* edge_dst /*[E]*/, int64_t E, const float* grad_out /*[N,out]*/,
                          int32_t out_features, float* grad_edge_w /*[E,out]*/, recon_stream_t stream);
/* out[k,:] = table[idx2[k,0],:] + table[idx2[k,1],:] — the n-hop relation embedding `relation_embed[edge_type_nhop[:, 0]] +
 * relation_embed[edge_type_nhop[:, 1]]` (GAT/models.py:64-65, 80-81) in one pass; the indices are the caller's to validate
 * (0 <= idx2 < table rows); its gradient is recon_spmm_rowsum_mod_fwd over the keys (idx2[:,0] | idx2[:,1]) */
int recon_gather_rows_pair_fwd(const float* table /*[rows,width]*/, const int64_t* idx2 /*[E,2]*/, int64_t E, int32_t width,
                               float* out /*[E,width]*/, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * G4  SpGraphAttentionLayer.forward for H heads that share inputs (GAT/layers.py:111-178; the
 *     head loop is GAT/models.py:71-72).  H = 1 is the single reference layer.
 *
 *   m_e   = A_dst x[dst_e] + A_src x[src_e] + A_rel r_e        a = [A_dst | A_src | A_rel]
 *   s_e   = a_2 . m_e ;  w_e = exp(-leakyrelu_alpha(s_e))      (no max subtraction)
 *   Z_i   = sum_{e: dst_e = i} w_e ;  Z_i == 0 -> 1e-12
 *   out_i = act( sum_e k_e w_e m_e / Z_i )                      k = dropout factors (after the row sum)
 *
 * Internals (caller-allocated, reused by the backward):
 *   P  [2][H][N][D]  projected node features (dst half, src half), head-major
 *   Q  [H][E][D]     projected edge features in CSR-slot order, head-major
 * ------------------------------------------------------------------------------------------*/
typedef struct {
    int32_t N, E;               /* must equal graph->N, graph->E                             */
    int32_t F, R, D, H;         /* in_features, nrela_dim, out_features per head, heads      */
    int32_t concat;             /* 1: ELU on the output (GAT/layers.py:173-175)              */
    float alpha;                /* LeakyReLU negative slope                                  */
    const float* x;             /* [N,F]                                                     */
    const float* edge_embed;    /* [E,R] rows in ORIGINAL edge order (1-hop rows then n-hop) */
    const float* a;             /* [H,D,2F+R]                                                */
    const float* a_2;           /* [H,D]                                                     */
    const float* keep;          /* [H,E] dropout factors in CSR-slot order, or NULL (eval)   */
    float* P;                   /* [2,H,N,D] workspace / saved                               */
    float* Q;                   /* [H,E,D]   workspace / saved                               */
    float* sigma;               /* [H,E] saved scores s_e (CSR-slot order); NULL iff Z NULL  */
    float* Z;                   /* [H,N] saved clamped row sums; NULL = inference call       */
    float* out;                 /* [N, ld_out] ; head h writes columns [h*D, (h+1)*D)        */
    int32_t ld_out;             /* >= H*D                                                    */
} recon_gat_fwd_args;

int recon_gat_fwd(const recon_graph* g, const recon_gat_fwd_args* args, recon_stream_t stream);

/* the two stages of recon_gat_fwd, exported for profiling / tests.
 * recon_gat_edge_fwd reads P, Q, a_2 (and keep) and writes out (and sigma, Z); x, a (and edge_embed where E > 0) must be non-NULL
 * but are not read.
 * Load width: VEC = 4 floats where D % 4 == 0, P, Q, a_2 and out are 16-byte aligned and ld_out % 4 == 0; VEC = 2 where the same holds
 * for D % 2, 8 bytes and ld_out % 2; else VEC = 1 (recon_gat_bwd: also grad_out, ld_gout, Gm, gP and partial).  A (node, head) row is
 * held by at most 64 lanes x 8 register rows of VEC floats: D <= 2048 / 1024 / 512 at VEC 4 / 2 / 1, RECON_ERR_UNSUPPORTED above
 * (nothing is launched, nothing written). */
int recon_gat_project(const recon_graph* g, const recon_gat_fwd_args* args, recon_stream_t stream); /* K4: MFMA */
int recon_gat_edge_fwd(const recon_graph* g, const recon_gat_fwd_args* args, recon_stream_t stream); /* K1: HBM  */
/* the edge kernel instance (csrc/gat.hip: k_gat_edge_fwd / k_gat_edge_bwd / k_gat_src_gather<VEC, G, KR>) a head width selects:
 * vec * 10000 + g * 100 + kr (vec: load width, g: lanes per (node, head) group, kr: register rows per lane), -1 where none exists.
 * align_floats is 4, 2 or 1: what the pointers and leading dimensions of the call allow (see above).  Host only. */
int32_t recon_gat_edge_instance(int32_t D, int32_t align_floats);

/* --------------------------------------------------------------------------------------------
 * K2  backward of recon_gat_fwd (autograd of GAT/layers.py:111-178 incl. the custom backward at
 *     :67-79; formulas in SURVEY.md appendix B).
 * ------------------------------------------------------------------------------------------*/
typedef struct {
    recon_gat_fwd_args fwd;     /* same tensors as the forward call (P, Q, sigma, Z, out filled) */
    const float* grad_out;      /* [N, ld_gout]                                              */
    int32_t ld_gout;
    float* Gm;                  /* [H,E,D]   workspace: d loss / d m_e, CSR-slot order       */
    float* gP;                  /* [2,H,N,D] workspace: d loss / d P                         */
    float* partial;             /* workspace, recon_gat_bwd_partial_floats() floats          */
    float* g_x;                 /* [N,F]      or NULL                                        */
    float* g_edge_embed;        /* [E,R] original edge order, or NULL                        */
    float* g_a;                 /* [H,D,2F+R] or NULL                                        */
    float* g_a_2;               /* [H,D]      or NULL                                        */
} recon_gat_bwd_args;

size_t recon_gat_bwd_partial_floats(int32_t N, int32_t E, int32_t F, int32_t R, int32_t D, int32_t H);
int recon_gat_bwd(const recon_graph* g, const recon_gat_bwd_args* args, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * G4'  the same layer in "aggregate, then project" order (csrc/gat_atp.hip).  Aggregation and
 *      projection are both linear, so  h_i = a . V_i  with
 *        V_i = [ x_i Zk_i/Z_i ; sum_e k_e w_e x[src_e] / Z_i ; sum_e k_e w_e r_e / Z_i ]   (2F+R per head)
 *      and the scores need only u = a_2^T a:  s_e = u_dst.x[dst_e] + u_src.x[src_e] + u_rel.r_e.
 *      Half the MFMA work of recon_gat_fwd when E = 4N and no [E, H*D] intermediate; results differ
 *      from recon_gat_fwd / the reference in fp32 summation order only.  recon_gat_atp_supported()
 *      tells whether the shape is instantiated (F, R even; 2F+R-wide rows fit the register budget).
 * ------------------------------------------------------------------------------------------*/
enum { RECON_SPLIT_BF16X3 = 0, RECON_SPLIT_F16X2 = 2 };

typedef struct {
    int32_t N, E;               /* must equal graph->N, graph->E                             */
    int32_t F, R, D, H;
    int32_t concat;
    float alpha;
    const float* x;             /* [N,F]                                                     */
    const float* edge_embed;    /* [E,R] original edge order                                 */
    const float* a;             /* [H,D,2F+R]                                                */
    const float* a_2;           /* [H,D]                                                     */
    const float* keep;          /* [E,H] dropout factors, CSR-slot order, or NULL            */
    float* u;                   /* [H,2F+R]  workspace / saved: a_2^T a                      */
    float* c_node;              /* [N,2H]    workspace / saved: x.u_dst | x.u_src            */
    float* c_rel;               /* [E,H]     workspace / saved: r_e.u_rel, CSR-slot order    */
    float* V;                   /* [N,H,2F+R] workspace / saved                              */
    float* sigma;               /* [E,H] saved scores (CSR-slot order); NULL iff Z NULL      */
    float* Z;                   /* [N,H] saved clamped row sums; NULL = inference call       */
    float* Zk;                  /* [N,H] saved sum_e k_e w_e                                 */
    float* out;                 /* [N, ld_out]; with a row-compacted graph (recon_graph.n_rows > 0): [n_rows, ld_out], row r = node row_node[r] */
    int32_t ld_out;
    void* a_split;              /* recon_gat_atp_split_bytes() bytes, workspace / saved: the three   *
                                 * bfloat16 term planes of a and a^T for the split-precision GEMMs   *
                                 * (csrc/gemm_bx3.hip; filled by the scores stage, read by the       *
                                 * projection and by the backward's g_V product).  NULL = use the    *
                                 * fp32-MFMA GEMM for those products.                                */
    int32_t split_mode;         /* RECON_SPLIT_*: which split-precision family a_split is for.  With         *
                                 * RECON_SPLIT_F16X2 (csrc/gemm_hx2.hip; needs (2F+R) % 8 == 0, D % 8 == 0,  *
                                 * else the call falls back to BF16X3) the buffers keep their sizes but hold  *
                                 * HALF planes: a_split the two planes of a and a^T, V the two planes         *
                                 * [2][N*H][2F+R] of s_V * V instead of fp32 V (head-major rows; when keep is  *
                                 * NULL the first F columns exist for head 0 only — they are the same for all  *
                                 * heads — and V is an opaque workspace), gh_split the two planes of g_h        */
    float keep_max;             /* upper bound of the factors in `keep` (1/(1-p)); ignored when keep is NULL  */
    void* aux;                  /* RECON_SPLIT_F16X2: recon_hx2_aux_bytes() bytes, 256-byte aligned, workspace *
                                 * / saved: max-magnitude slots of a, x, edge_embed, grad_out (the per-tensor   *
                                 * power-of-two scales derive from them) and a page of zeros; zeroed by the     *
                                 * scores stage; the backward publishes grad_out's slots and re-zeroes them     *
                                 * in its last kernel, so it must be given the aux of the matching forward      */
    const int32_t* ee_index;    /* NULL: edge_embed holds one row per edge.  Else [E], CSR-slot order: edge_embed is a TABLE and the *
                                 * edge in slot k uses row ee_index[k] of it — `relation_embed[edge_type]` (GAT/models.py:156, :79)  *
                                 * read in place instead of materialised as E x R; n-hop edges index rows appended to the table.      *
                                 * The backward then writes g_edge_embed [E,R] in CSR-SLOT order (row k = gradient of the row slot k    *
                                 * used); summing those rows by ee_index gives the table's gradient (recon_spmm_rowsum_fwd).            */
    int32_t ee_rows;            /* rows of the table when ee_index is set (ignored otherwise).  c_rel then holds max(E, ee_rows) x H    *
                                 * floats: the score terms r.u_rel are computed once per table ROW and looked up per edge               */
    int32_t io_bf16;            /* 1: x [N,F] and edge_embed [E,R] are BFLOAT16 (same shapes, 8-byte aligned) and the forward's kernels   *
                                 * read them in place (BASELINE.json configs[4]: "mixed GAT+Propagation stack, bf16"; everything else     *
                                 * of the call is unchanged: fp32 arithmetic, fp32 out).  Forward calls only (scores, aggregate,          *
                                 * project), shapes of recon_gat_atp_bf16_io_supported(), no ee_index; the backward takes fp32 copies.    */
} recon_gat_atp_args;
int recon_gat_atp_bf16_io_supported(int32_t F, int32_t R, int32_t D, int32_t H);

size_t recon_gat_atp_split_bytes(int32_t F, int32_t R, int32_t D, int32_t H);
/* 1 if the RECON_SPLIT_F16X2 mode takes this shape ((2F+R) % 8 == 0, D % 8 == 0, plane offsets within 32 bits); given that,
 * 16-byte aligned a_split / V, 256-byte aligned aux and ld_out % 4 == 0 the call uses it, otherwise it falls back to BF16X3 */
int recon_gat_atp_f16x2_supported(int32_t F, int32_t R, int32_t D, int32_t H);
int recon_gat_atp_supported(int32_t N, int32_t E, int32_t F, int32_t R, int32_t D, int32_t H);
/* the edge-pass kernel instance the widths select: vec * 1000 + kr * 10 + log2(ht) (vec: load width, kr: register rows per lane,
 * ht: heads per wave), -1 where no instance exists.  Host only; says nothing about the other limits of recon_gat_atp_supported() */
int32_t recon_gat_atp_instance(int32_t F, int32_t R, int32_t H);
int recon_gat_atp_fwd(const recon_graph* g, const recon_gat_atp_args* args, recon_stream_t stream);
/* the three stages of recon_gat_atp_fwd, exported for profiling / tests */
int recon_gat_atp_scores(const recon_graph* g, const recon_gat_atp_args* args, recon_stream_t stream);    /* u, c_node, c_rel */
int recon_gat_atp_aggregate(const recon_graph* g, const recon_gat_atp_args* args, recon_stream_t stream); /* K1': HBM       */
int recon_gat_atp_project(const recon_graph* g, const recon_gat_atp_args* args, recon_stream_t stream);   /* K4: MFMA       */

typedef struct {
    recon_gat_atp_args fwd;     /* same tensors as the forward call (u, V, sigma, Z, Zk, out filled)  */
    const float* grad_out;      /* [N, ld_gout] — all nodes, also with a row-compacted graph (rows are read through row_node)        */
    int32_t ld_gout;
    float* g_h;                 /* [N,H*D]    workspace (written when concat != 0 or the graph is row-compacted; unused, may be NULL, in F16X2 mode) */
    float* g_V;                 /* [N,H,2F+R] workspace: d loss / d V                                 */
    float* g_sigma;             /* [E,H]      workspace: d loss / d s_e                               */
    float* Gxs;                 /* [E,F]      workspace: per-edge gradient rows bound for x[src_e]    */
    float* gxd;                 /* [N,F]      workspace: destination-side part of d loss / d x        */
    float* Gs;                  /* [N,2H]     workspace: per-node sums of g_sigma (dst view | src view) */
    float* g_u;                 /* [H,2F+R]   workspace: d loss / d (a_2^T a)                          */
    float* q;                   /* [N,H]      workspace: g_h . h per (node, head)                      */
    float* partial;             /* workspace, recon_gat_atp_bwd_partial_floats() floats (split-K)     */
    float* partial2;            /* workspace, recon_gat_atp_bwd_partial2_floats() floats (skinny)     */
    float* g_x;                 /* [N,F]      or NULL                                                 */
    float* g_edge_embed;        /* [E,R] original edge order, or NULL                                 */
    float* g_a;                 /* [H,D,2F+R] or NULL (then g_a_2 must be NULL too)                    */
    float* g_a_2;               /* [H,D]      or NULL                                                 */
    void* gh_split;             /* recon_gat_atp_bwd_split_bytes() bytes, workspace: bfloat16 term planes of g_h for  *
                                 * the split-precision weight-gradient GEMM; NULL (or fwd.a_split NULL) = fp32 MFMA  */
    int32_t g_ee_bf16;          /* 1: g_edge_embed points to BFLOAT16 rows [E,R] — the edge pass rounds its fp32 sums once, where it stores  *
                                 * them (fwd.io_bf16 callers whose edge embeddings take a bfloat16 gradient: 116 MB written as fp32 and    *
                                 * re-read by a cast at BASELINE.json configs[4]).  Only where recon_gat_atp_bwd_gee_bf16_supported() says 1  */
} recon_gat_atp_bwd_args;
/* whether g_ee_bf16 = 1 is available for these widths: fwd.io_bf16 shapes whose heads are walked in ONE group per wave (a second head group
 * adds to the rows the first one stored: that sum has to stay fp32) */
int recon_gat_atp_bwd_gee_bf16_supported(int32_t F, int32_t R, int32_t D, int32_t H);

size_t recon_gat_atp_bwd_split_bytes(int32_t N, int32_t D, int32_t H);

size_t recon_gat_atp_bwd_partial_floats(int32_t N, int32_t E, int32_t F, int32_t R, int32_t D, int32_t H);
size_t recon_gat_atp_bwd_partial2_floats(int32_t N, int32_t E, int32_t F, int32_t R, int32_t D, int32_t H);
/* Host only: the launch plan of the backward's last three kernels for a shape (NR: destination rows, N unless the graph is
 * row-compacted).  plan[0..2]: row slices of the three skinny products (destination sums over NR rows, source sums over N rows, the
 * edge-side product over E rows; 0 for a product without rows), plan[3..5]: blocks of their fixed-order reduce (16 elements each),
 * plan[6]: splits of the weight gradient V^T g_h, plan[7]: its tile workgroups, plan[8]: the z extent of its grid with the reduce's
 * plan[9] blocks riding in further layers behind the tiles.
 * Returns 1 where the reduce rides in the weight gradient's launch — the F16X2 mode with per-row scales (D <= 256), at most 8 heads,
 * in a recon_gat_atp_bwd call (or a phase call with INPUTS and WEIGHTS and without EARLY_SUM) on a graph without source-side hub
 * pieces —, 0 where it keeps a launch of its own. */
int recon_gat_atp_bwd_ride_plan(int32_t NR, int32_t N, int32_t E, int32_t F, int32_t R, int32_t D, int32_t H, int32_t* plan /*[10]*/);
int recon_gat_atp_bwd(const recon_graph* g, const recon_gat_atp_bwd_args* args, recon_stream_t stream);
/* the same backward as independently launchable phases (bit mask): PREPARE -> { INPUTS, WEIGHTS } -> FINISH.
 * INPUTS (g_V GEMM, edge pass, source pass, score-vector gradient: HBM bound) and WEIGHTS (g_a = g_h^T V:
 * MFMA bound) only read what PREPARE wrote and touch disjoint workspaces, so they may run on two streams. */
enum { RECON_ATP_BWD_PREPARE = 1, RECON_ATP_BWD_INPUTS = 2, RECON_ATP_BWD_WEIGHTS = 4, RECON_ATP_BWD_FINISH = 8,
       RECON_ATP_BWD_ALL = 15,
       /* modifier for data-parallel callers that reduce the weight gradient across ranks UNDER the INPUTS phase: with WEIGHTS, the
        * split-K second pass runs at once and leaves g_a = G = V^T g_h (the part of g_a that does not depend on INPUTS); with FINISH,
        * g_a is taken to hold G already and only  g_a += a_2 (x) g_u,  g_a_2 = a . g_u  are applied.  Both are linear in (G, g_u), so
        * mean over ranks of g_a = mean(G) + a_2 (x) mean(g_u): all-reduce G early, g_u (H x (2F+R) floats) after INPUTS, then FINISH. */
       RECON_ATP_BWD_EARLY_SUM = 16 };
int recon_gat_atp_bwd_phase(const recon_graph* g, const recon_gat_atp_bwd_args* args, int32_t phases,
                            recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * P1  block adjacency of the GP-GNN step (models/models.py:240-259; copies :450-469, :660-679,
 *     :898-917):  A[b, i*dd+r, j*dd+c] = T[b, e(i,j), r*dd+c] for i != j (e = row-major over ordered
 *     pairs, diagonal skipped) and identity[r,c] for i == j;  dd = 2*embedding_dim, S = n*dd.
 *     T is the per-pair transition tensor AFTER the non-linearity, [B, n(n-1), dd*dd].
 * ------------------------------------------------------------------------------------------*/
int recon_block_adjacency_fwd(const float* T, const float* identity, int32_t B, int32_t n, int32_t dd,
                              float* A /*[B,S,S]*/, recon_stream_t stream);
/* gT [B,n(n-1),dd*dd] and g_identity [dd,dd] (either may be NULL) from gA [B,S,S]; `workspace`
 * (recon_block_adjacency_bwd_workspace_floats() floats) holds the per-slice partial sums of g_identity, which
 * is reduced in a fixed order (required when g_identity is not NULL). */
size_t recon_block_adjacency_bwd_workspace_floats(int32_t B, int32_t n, int32_t dd);
int recon_block_adjacency_bwd(const float* gA, int32_t B, int32_t n, int32_t dd, float* gT, float* g_identity,
                              float* workspace, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * P2 / K5  L-hop gated propagation + head*tail gather (models/models.py:260-274; copies :470-485,
 *     :680-694, :918-932):  h^0 = h0;  h^l = act(A_l h^l-1)  per channel c;
 *     out[b, c, l*dd + x] = h^l[b, c, head[c,x]] * h^l[b, c, tail[c,x]].
 *     One launch runs all L hops with the channel states resident in LDS (MFMA 16x16x4 fp32).
 * ------------------------------------------------------------------------------------------*/
enum { RECON_ACT_LINEAR = 0, RECON_ACT_RELU = 1, RECON_ACT_TANH = 2 };
typedef struct {
    int32_t B, C, S, L, dd;         /* graphs, channels n(n-1), state size n*dd, hops, gather width      */
    int32_t act;                    /* RECON_ACT_*  (model_params.json "non-linear1")                    */
    const float* const* adj;        /* HOST array of L device pointers, each [B,S,S]                     */
    const float* h0;                /* [C,S] shared (h0_batch_stride = 0) or [B,C,S] (stride = C*S)       */
    int64_t h0_batch_stride;
    const int64_t* head_idx;        /* [C,dd] (idx_batch_stride = 0) or [B,C,dd]; values in [0,S)         */
    const int64_t* tail_idx;
    int64_t idx_batch_stride;
    float* out;                     /* [B,C,L*dd]                                                         */
    float* h_saved;                 /* [L,B,C,S] states after each hop (for the backward) or NULL         */
    const float* const* trans;      /* BLOCK MODE (or NULL): HOST array of L device pointers, each [B, n(n-1), dd*dd] — the  *
                                     * transition matrices AFTER the non-linearity; A_l is then never materialised: the     *
                                     * kernels read A_l[b, i*dd+r, j*dd+c] = trans[l][b, e(i,j), r, c] (identity[r,c] on the   *
                                     * diagonal blocks) in place, recon_block_adjacency_fwd's layout.  `adj` is ignored.    *
                                     * Only where recon_propagate_form() == 1 and dd == 16 (S = 16 n).                      */
    const float* identity;          /* [dd,dd], with trans                                                               */
    float* stats;                   /* [B, 2L+1] or NULL: per graph the max magnitudes of h^0..h^L and of   *
                                     * A_1..A_L.  Written by the forward when h_saved is given and          *
                                     * recon_propagate_form() == 1 (the two-term f16 kernels, whose         *
                                     * per-tensor scales in the backward come from these); the backward     *
                                     * runs its two-term form only when given the same buffer              */
    void* split_ws;                 /* recon_propagate_ws_bytes() bytes or NULL.  Wide states (160 < S <= 512, e.g. 32 nodes *
                                     * at 2d = 16): with it the forward runs the two-term f16 form of csrc/prop_hl.hip (A_l  *
                                     * pre-split into half terms per slice of graphs, 64-channel chunks per workgroup);      *
                                     * without it, the fp32 matrix-core form                                                 */
    int64_t split_ws_bytes;
} recon_prop_args;

int recon_propagate_fwd(const recon_prop_args* args, recon_stream_t stream);
/* Bit 0: the forward of this problem runs on the two-term f16 matrix-core kernels (csrc/prop_h.hip: S % 16 == 0, S <= 160, C <= 96,
 * aligned pointers, RECON_PROP_FWD unset or "h"); bit 1: so does the backward (its LDS image also fits); 0: fp32 matrix-core forms.
 * Block mode (`trans`) needs both bits when gradients are wanted.  The adjacency pointers need not be set for this query. */
int recon_propagate_form(const recon_prop_args* args);
/* Bytes of `split_ws` that let recon_propagate_fwd run the wide-state two-term form for this problem (B, S, L; block mode or not),
 * 0 where that form does not exist (S <= 160: the whole graph fits one workgroup and needs no workspace; S > 512). */
size_t recon_propagate_ws_bytes(const recon_prop_args* args);

typedef struct {
    recon_prop_args fwd;            /* h_saved filled by the forward call                                 */
    const float* grad_out;          /* [B,C,L*dd]                                                         */
    float* const* g_adj;            /* HOST array of L device pointers [B,S,S] (entries may be NULL)      */
    float* g_h;                     /* [B,C,S] workspace; on return holds d loss / d h0 per batch element */
    float* const* g_trans;          /* block mode: HOST array of L device pointers [B, n(n-1), dd*dd] (entries may be NULL): *
                                     * the gradient lands in the transition tensors' own layout, g_adj is ignored           */
    float* g_identity;              /* block mode: [dd,dd] summed over graphs, nodes and hops (fixed order), or NULL         */
    float* identity_ws;             /* block mode: recon_propagate_identity_ws_floats() floats when g_identity is wanted    */
    float* wide_ws;                 /* recon_propagate_bwd_ws_floats() floats or NULL.  Wide states (S > 160): with it both products *
                                     * of a hop run as batched GEMMs over the graphs; without it, the channel-chunked kernel         */
    const int32_t* head_blk;        /* [C] device or NULL: the gather indices are BLOCKS of 16 consecutive columns (head_idx[c, x] =   *
                                     * head_blk[c] + x, likewise tail; dd = 16, block starts multiples of 16, head and tail blocks of  *
                                     * a channel distinct, idx_batch_stride = 0 — what utils/embedding_utils.py:184-202 builds; the    *
                                     * caller has checked it).  With chain_ws and fwd.split_ws the wide backward then runs its chain   *
                                     * d loss / d H^l-1 = A_l^T Y_l on the forward's two-term f16 kernel, all hops in one launch       */
    const int32_t* tail_blk;
    float* chain_ws;                /* recon_propagate_bwd_chain_ws_floats() floats or NULL                                            */
} recon_prop_bwd_args;

size_t recon_propagate_identity_ws_floats(int32_t dd);
size_t recon_propagate_bwd_ws_floats(const recon_prop_args* fwd);   /* B*C*S for S > 160 (not in block mode), else 0 */
size_t recon_propagate_bwd_chain_ws_floats(const recon_prop_args* fwd);   /* L * (graphs per slice) * C * S where the chain form exists (160 < S <= 512, dd = 16, shared indices, fwd.split_ws set), else 0 */

int recon_propagate_bwd(const recon_prop_bwd_args* args, recon_stream_t stream);

/* Which kernel instance a call launches: recon_propagate_instance() for recon_propagate_fwd(args), recon_propagate_bwd_instance() for
 * recon_propagate_bwd(args) (the backward's choice depends on the workspaces of recon_prop_bwd_args, hence its own entry).  Computed by
 * the code the launchers dispatch on, RECON_PROP_* switches included; host arithmetic only: no device is needed and the pointers are
 * looked at for null and for alignment, never followed (the HOST arrays adj / trans / g_adj / g_trans are read).
 * Returns -1 where the call would be refused, 0 where it launches nothing (B == 0), else
 *     key = family * 10000 + p1 * 100 + p2 * 10 + flag
 *     family  kernel(s)                                                        p1    p2    flag
 *        1    k_propagate_fwd_h / k_propagate_bwd_h (two-term f16, S <= 160)   NKS   NTC   block mode
 *        2    k_propagate_fwd_hl (two-term f16, wide states)                   NKS   RT    block mode
 *        3    k_propagate_fwd_hl<.., true> chain + k_prop_gadj_hl<RT, 8>       NKS   RT    block mode       (backward)
 *        4    the same with k_prop_gadj_hl<RT, 16> (C > 256)                   NKS   RT    block mode       (backward)
 *        5    k_propagate_fwd_w (fp32 MFMA, state in registers per wave)       NTn   0     V4 (float4 loads of A_l)
 *        6    k_propagate_fwd (fp32 MFMA, state in LDS per workgroup)          MT    0     V4
 *        7    k_propagate_bwd_hop (fp32 MFMA, one launch per hop)              MT    0     V4 (float4 staging of the states) (backward)
 *        8    batched fp32 GEMMs + k_prop_bwd_post (wide states)               0     0     0                (backward)
 * e.g. 10340 = k_propagate_fwd_h<3, 4, false>, 50901 = k_propagate_fwd_w<9, true>. */
int32_t recon_propagate_instance(const recon_prop_args* args);
int32_t recon_propagate_bwd_instance(const recon_prop_bwd_args* args);

/* --------------------------------------------------------------------------------------------
 * P1 / P2 / K5 in bfloat16 (BASELINE.json configs[2] "GP-GNN Propagation 3 hops ... bf16", configs[4] "mixed GAT+Propagation
 *     stack, bf16"): the same step (models/models.py:240-274) on bfloat16 tensors — bf16 storage, fp32 accumulation on
 *     v_mfma_f32_16x16x32_bf16, every state and every gradient tensor rounded to bf16 once where the reference's bf16 tensors
 *     are (csrc/prop_b16.hip).  All data pointers are bf16 (uint16_t) data, 16-byte aligned, S % 8 == 0.
 *     recon_propagate_b16_form(): 1 = all hops of a graph in one workgroup (S % 16 == 0, S <= 160, C <= 96, even dd; h_saved
 *     optional), 3 = wide states (S % 64 == 0, 192 <= S <= 512): the state of 128 channels in LDS for all hops, 2 = one batched GEMM
 *     per hop over the graphs (needs h_saved and `zeros`), 0 = shape not taken (the caller converts to float32 and runs
 *     recon_propagate_fwd).  Every form reads `trans` in place in block mode.
 *     The backward runs both products of a hop as batched GEMMs over the graphs for every shape, in block mode without an adjacency.
 * ------------------------------------------------------------------------------------------*/
typedef struct {
    int32_t B, C, S, L, dd;         /* as recon_prop_args                                                 */
    int32_t act;                    /* RECON_ACT_*                                                        */
    const void* const* adj;         /* HOST array of L device pointers, each [B,S,S] bf16 (ignored with trans) */
    const void* h0;                 /* [C,S] (h0_batch_stride = 0) or [B,C,S] bf16                        */
    int64_t h0_batch_stride;        /* elements; multiple of 8                                            */
    const int64_t* head_idx;        /* [C,dd] (idx_batch_stride = 0) or [B,C,dd]; values in [0,S)         */
    const int64_t* tail_idx;
    int64_t idx_batch_stride;
    void* out;                      /* [B,C,L*dd] bf16                                                    */
    void* h_saved;                  /* [L,B,C,S] bf16 states after each hop: for the backward; required by form 2 */
    const void* const* trans;       /* BLOCK MODE (form 1 only) or NULL: L device pointers [B, n(n-1), 256] bf16 */
    const void* identity;           /* [16,16] bf16, with trans                                           */
    const void* zeros;              /* >= 1 KiB of zero bytes, 16-byte aligned (K tails of the GEMMs): form 2 and the backward */
} recon_prop_b16_args;

int recon_propagate_b16_form(const recon_prop_b16_args* args);
int recon_propagate_b16_fwd(const recon_prop_b16_args* args, recon_stream_t stream);

typedef struct {
    recon_prop_b16_args fwd;        /* adj or trans + identity, h_saved (filled by the forward), zeros    */
    const void* grad_out;           /* [B,C,L*dd] bf16                                                    */
    void* const* g_adj;             /* HOST array of L device pointers [B,S,S] bf16 (entries may be NULL) */
    void* g_h;                      /* [B,C,S] bf16; on return d loss / d h0 per batch element            */
    void* ws;                       /* [B,C,S] bf16 workspace                                             */
    const int32_t* head_blk;        /* [C] device or NULL: the gather indices are BLOCKS of dd consecutive columns (head_idx[c, x] =     *
                                     * head_blk[c] + x, likewise tail; what utils/embedding_utils.py:184-202 builds) — the caller has   *
                                     * checked it, idx_batch_stride == 0, head_blk[c] != tail_blk[c]: Y_l is then formed in the GEMM   *
                                     * epilogues instead of by a pass of its own                                                        */
    const int32_t* tail_blk;
    void* const* g_trans;           /* BLOCK MODE (fwd.trans): HOST array of L device pointers [B, n(n-1), 256] bf16 (entries may be NULL) */
    void* g_identity;               /* block mode: [16,16] bf16 summed over graphs, nodes and hops (fp32, fixed order), or NULL          */
    void* diag_ws;                  /* block mode with g_identity: recon_propagate_b16_bwd_diag_elems() bf16 elements                   */
    float* ident_ws;                /* block mode with g_identity: recon_block_adjacency_b16_bwd_workspace_floats(16) floats            */
} recon_prop_b16_bwd_args;

size_t recon_propagate_b16_bwd_diag_elems(const recon_prop_b16_args* fwd);
int recon_propagate_b16_bwd(const recon_prop_b16_bwd_args* args, recon_stream_t stream);
/* recon_propagate_instance() for the bfloat16 calls, same key layout and rules.  backward == 0: what recon_propagate_b16_fwd(args) launches,
 *     family 11  k_prop_b16_fwd (form 1)        p1 = NKS, p2 = NTC, flag = block mode
 *     family 12  k_prop_b16_fwd_wide (form 3)   p1 = NKS, p2 = RT,  flag = block mode
 *     family 13  one k_bgemm_b16 product per hop + gather (form 2); flag = block mode
 * backward != 0: 140000 + block mode (k_bgemm_b16 products for every shape) where recon_propagate_b16_bwd takes the forward's arguments
 * (16-byte aligned gradient buffers assumed), -1 where it refuses them. */
int32_t recon_propagate_b16_instance(const recon_prop_b16_args* args, int32_t backward);

/* P1 in bf16: recon_block_adjacency_fwd / _bwd on bf16 tensors (the identity gradient is summed in fp32, fixed order, rounded once) */
int recon_block_adjacency_b16_fwd(const void* T, const void* identity, int32_t B, int32_t n, int32_t dd, void* A, recon_stream_t stream);
size_t recon_block_adjacency_b16_bwd_workspace_floats(int32_t dd);
int recon_block_adjacency_b16_bwd(const void* gA, int32_t B, int32_t n, int32_t dd, void* gT, void* g_identity, float* workspace,
                                  recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * The GAT_sep_space variant's entity -> relation-space map (GAT_sep_space/main.py:359-364, :372-377; GAT_sep_space/models.py:316-320):
 *     out[t] = x[t] . W[rel[t]]      x [T, in_dim], W [R, in_dim, out_dim], rel [T] in [0, R)
 * without the [T, in_dim, out_dim] gather the reference feeds to torch.bmm.  `order` [T] int32 = the rows in relation order (a stable
 * argsort of rel), `seg_ptr` [R+1] int32 = where each relation's rows start in that order.  transpose_w: W is [R, out_dim, in_dim] and
 * read transposed (the input gradient g_x[t] = g[t] . W[rel[t]]^T).  _wgrad: g_W[r] = sum over the rows t of relation r of x[t]^T g[t]
 * (dense [R, in_dim, out_dim]: relations without rows get zeros), fixed summation order.  in_dim <= 1024, out_dim <= 512 for _wgrad.
 * ------------------------------------------------------------------------------------------*/
int recon_rel_rows_mm(const float* x, const int32_t* order, const int64_t* rel, const float* W, int32_t T, int32_t in_dim, int32_t out_dim,
                      int32_t transpose_w, float* out, recon_stream_t stream);
int recon_rel_rows_mm_wgrad(const float* x, const float* g, const int32_t* order, const int32_t* seg_ptr, int32_t R, int32_t in_dim,
                            int32_t out_dim, float* gW, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * P4  make_start_entity_embeddings (utils/context_utils.py:387-426): h0[b,c=(i,j),:] has the first
 *     entity's embedding in node i's first half-slot and the second entity's in node j's second
 *     half-slot, zero elsewhere, times the start-embedding template.
 * ------------------------------------------------------------------------------------------*/
int recon_start_entity_embeddings(const float* entity_embeddings /*[U,d]*/, const int64_t* pos /*[B,C,2]*/,
                                  const float* templ /*[C,S]*/, int32_t B, int32_t n, int32_t d,
                                  float* out /*[B,C,S]*/, recon_stream_t stream);
/* Its backward, first half (the reference has none of its own: autograd's index_put_ backward of context_utils.py:413-420, whose
 * float atomics fix no summation order): rows [2][B*C][d] = the d-wide pieces of (grad_out * templ) that belong to pos[..., 0]
 * (node i's first half-slot) and pos[..., 1] (node j's second half-slot), and — when `key` is given — key [2][2*B*C] = those entity
 * ids twice (the [2, E] segment key of recon_spmm_rowsum_fwd over a destination-only recon_graph: the fixed-order second half). */
int recon_start_entity_embeddings_bwd(const float* grad_out /*[B,C,S]*/, const int64_t* pos /*[B,C,2]*/, const float* templ /*[C,S]*/,
                                      int32_t B, int32_t n, int32_t d, float* rows /*[2,B*C,d]*/, int64_t* key /*[2,2*B*C] or NULL*/,
                                      recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * P5 / K6  GraphConvolution (models/layers.py:57-63), batched over B graphs (B = 1 is the
 *     reference's 2-D call):  out = relu(adj @ (x @ W) + bias).
 *     support [B*n,out] is caller-allocated scratch / saved for the backward.
 * ------------------------------------------------------------------------------------------*/
typedef struct {
    int32_t B, n, in_features, out_features;
    const float* x;                 /* [B,n,in]   */
    const float* adj;               /* [B,n,n]    */
    const float* weight;            /* [in,out]   */
    const float* bias;              /* [out] or NULL */
    float* support;                 /* [B,n,out]  x @ W */
    float* out;                     /* [B,n,out]  */
    void* w_split;                  /* recon_gcn_split_bytes() bytes or NULL: bfloat16 term planes of W^T and W *
                                     * (filled by recon_gcn_fwd, read again by recon_gcn_bwd); with it x @ W and *
                                     * g_support @ W^T run on the split-precision GEMM (csrc/gemm_bx3.hip)       */
} recon_gcn_args;

size_t recon_gcn_split_bytes(int32_t in_features, int32_t out_features);
int recon_gcn_fwd(const recon_gcn_args* args, recon_stream_t stream);

typedef struct {
    recon_gcn_args fwd;
    const float* grad_out;          /* [B,n,out] */
    float* g_support;               /* [B,n,out] workspace */
    float* partial;                 /* workspace: recon_gcn_bwd_partial_floats() floats */
    float* g_x;                     /* [B,n,in]  or NULL */
    float* g_adj;                   /* [B,n,n]   or NULL */
    float* g_weight;                /* [in,out]  or NULL */
    float* g_bias;                  /* [out]     or NULL */
    void* gs_split;                 /* recon_gcn_bwd_split_bytes() bytes or NULL: bfloat16 term planes of g_support for *
                                     * the split-precision weight-gradient product (needs fwd.w_split as well)         */
} recon_gcn_bwd_args;

size_t recon_gcn_bwd_split_bytes(int32_t B, int32_t n, int32_t out_features);

size_t recon_gcn_bwd_partial_floats(int32_t B, int32_t n, int32_t in_features, int32_t out_features);
int recon_gcn_bwd(const recon_gcn_bwd_args* args, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * P5 / K6 over a RAGGED batch in float32 (BASELINE.json configs[4]: graphs of up to 256 nodes, every one its own size): graph b owns
 *     node rows node_ptr[b] .. node_ptr[b+1] of x / support / out (total_rows = node_ptr[B] rows in all, n_max the largest graph) and a
 *     dense n_b x n_b adjacency at adj + adj_ptr[b] (elements).  The layer of models/layers.py:57-63 applied to every graph: x @ W over
 *     all rows at once (the GEMMs of recon_gcn_fwd; w_split / gs_split as there, sized by recon_gcn_split_bytes(in, out) and
 *     recon_gcn_bwd_split_bytes(1, total_rows, out), or NULL), the aggregate per graph on v_mfma_f32_16x16x4_f32.
 *     x: rows of in_features floats at a stride of ldx >= in_features floats; adj, support, out, grad_out and the gradients are dense.
 *     tiles [n_tiles][2] int32, device: the work list (graph b, row tile i) for b = 0 .. B-1, i = 0 .. ceil(n_b / 32) - 1, in any
 *     order; a pair that names no graph or no rows of its graph is skipped.
 *     Plain arguments, no struct.  All sizes, pointers and counts are checked before anything is launched: RECON_ERR_INVALID for a null
 *     required pointer, in_features / out_features <= 0, ldx < in_features, sizes that no batch has (B == 0 with rows, n_max > total_rows,
 *     total_rows > B * n_max) or an n_tiles outside B .. (total_rows + 31 B) / 32; RECON_ERR_UNSUPPORTED for B > 65535, total_rows beyond
 *     int32 or n_max > 65535 * 32.  B == 0 launches nothing.  No atomics: results are bit-reproducible.
 * ------------------------------------------------------------------------------------------*/
/* The size checks alone (models/layers.py:57-63 per graph): RECON_OK where the two launchers below would take these sizes. */
int recon_gcn_ragged_supported(int32_t B, int64_t total_rows, int32_t n_max, int32_t in_features, int32_t out_features);
/* Forward, models/layers.py:57-63 per graph: support = x @ W (scratch / saved), out = relu(adj_b @ support_b + bias); bias may be NULL. */
int recon_gcn_ragged_fwd(const float* x, int64_t ldx, const float* adj, const float* weight, const float* bias, const int32_t* node_ptr,
                         const int64_t* adj_ptr, const int32_t* tiles, int32_t n_tiles, int32_t B, int64_t total_rows, int32_t n_max,
                         int32_t in_features, int32_t out_features, float* support, float* out, void* w_split, recon_stream_t stream);
/* Floats of the backward's `partial` (autograd's backward of models/layers.py:57-63): the weight gradient's split-K partials + [B, out]
 * per-graph column sums for the bias gradient. */
size_t recon_gcn_ragged_bwd_partial_floats(int32_t B, int64_t total_rows, int32_t in_features, int32_t out_features);
/* Backward (what autograd derives from models/layers.py:57-63, per graph): g_support [total_rows, out] workspace = adj_b^T @ (grad_out *
 * (out > 0)); g_x [total_rows, in], g_adj (laid out as adj; reads support), g_weight [in, out], g_bias [out]: each optional (NULL).
 * g_bias is the per-graph column sums of the masked gradient added in graph order.  support, out, w_split: as the forward left them. */
int recon_gcn_ragged_bwd(const float* x, int64_t ldx, const float* adj, const float* weight, const int32_t* node_ptr, const int64_t* adj_ptr,
                         const int32_t* tiles, int32_t n_tiles, int32_t B, int64_t total_rows, int32_t n_max, int32_t in_features,
                         int32_t out_features, const float* support, const float* out, const void* w_split, const float* grad_out,
                         float* g_support, float* partial, float* g_x, float* g_adj, float* g_weight, float* g_bias, void* gs_split,
                         recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * P5 / K6 in bfloat16 (BASELINE.json configs[2]: "bf16 + MFMA on W-projection"): the same layer on bfloat16 tensors — bf16
 *     storage, fp32 accumulation, x @ W / g_support @ W^T / x^T @ g_support on v_mfma_f32_16x16x32_bf16 (csrc/gemm_b16.hip).
 *     Activations carry a row stride that is a multiple of 8 elements (16 bytes) and at least the feature count rounded up
 *     to 8, so that feature counts like 300 need no repacking between layers; columns past the feature count of `support`,
 *     `out` and `g_support` are written as zeros, those of `x` must be finite.  All pointers are bf16 (uint16_t) data.
 * ------------------------------------------------------------------------------------------*/
typedef struct {
    int32_t B, n, in_features, out_features;
    const void* x; int64_t ldx;     /* [B*n, ldx] bf16, 16-byte aligned.  Fused forward (support == NULL): any even   *
                                     * ldx >= in_features — the kernel masks the K tail, so rows need no padding and *
                                     * whatever lies behind a row's last feature is never multiplied                 */
    const void* adj;                /* [B, n, n] bf16                                                            */
    const void* weight;             /* [in, out] bf16, contiguous                                                */
    const void* bias;               /* [out] bf16 or NULL                                                        */
    void* support; int64_t lds;     /* [B*n, lds] bf16: x @ W, scratch / saved                                    */
    void* out; int64_t ldo;         /* [B*n, ldo] bf16                                                           */
    void* w_planes;                 /* recon_gcn_b16_planes_bytes() bytes, scratch / saved: W^T and W zero padded along k */
    int32_t w_planes_valid;         /* != 0: w_planes already holds the planes of `weight` (a caller that keeps them across      *
                                     * calls while the weight is unchanged — inference — saves the two repacking launches)      */
    /* RAGGED batch (BASELINE.json configs[4]: graphs of up to 256 nodes each, every one its own size), or NULL / 0: graph b owns node  *
     * rows node_ptr[b] .. node_ptr[b+1] of x / support / out (total_rows = node_ptr[B] rows in all) and a dense n_b x n_b adjacency   *
     * at adj + adj_ptr[b] (elements); `n` is then the LARGEST n_b.  The layer of models/layers.py:57-63 applied to every graph:        *
     * x @ W over all rows at once, the aggregate per graph.  `support` is required.                                                    */
    const int32_t* node_ptr;        /* [B+1] device, ascending, node_ptr[0] = 0                                  */
    const int64_t* adj_ptr;         /* [B+1] device: adj_ptr[b] = sum over b' < b of n_b'^2                      */
    int64_t total_rows;
} recon_gcn_b16_args;

typedef struct {
    recon_gcn_b16_args fwd;
    const void* grad_out; int64_t ldg;   /* [B*n, ldg] bf16; ldg % 8 == 0 and >= out rounded up to 8                */
    void* g_support;                /* [B*n, fwd.lds] bf16 workspace, 16-byte aligned: fwd.lds % 8 == 0 and >= out *
                                     * rounded up to 8 also where the forward ran with support == NULL; columns    *
                                     * out .. fwd.lds are written as zeros                                          */
    float* partial;                 /* recon_gcn_b16_bwd_partial_floats() floats; ragged batch:                  *
                                     * recon_gcn_b16_bwd_partial_floats(1, total_rows, in, out) + B * out floats  */
    void* g_x; int64_t ldgx;        /* [B*n, ldgx] bf16 or NULL                                                  */
    void* g_adj;                    /* [B, n, n] bf16 or NULL; reads fwd.support (RECON_ERR_INVALID without it)   */
    void* g_weight;                 /* [in, out] bf16 or NULL; reads x in rows of fwd.ldx % 8 == 0 elements       */
    void* g_bias;                   /* [out] bf16 or NULL                                                        */
    const void* zeros;              /* >= 1 KiB of zero bytes, 16-byte aligned (K tails of the k-major GEMM)     */
} recon_gcn_b16_bwd_args;

size_t recon_gcn_b16_planes_bytes(int32_t in_features, int32_t out_features);
int recon_gcn_b16_fwd(const recon_gcn_b16_args* args, recon_stream_t stream);
size_t recon_gcn_b16_bwd_partial_floats(int32_t B, int32_t n, int32_t in_features, int32_t out_features);
int recon_gcn_b16_bwd(const recon_gcn_b16_bwd_args* args, recon_stream_t stream);

/* Which kernels a call launches: recon_gcn_b16_fwd_instance() for recon_gcn_b16_fwd(args), recon_gcn_b16_bwd_instance() for
 * recon_gcn_b16_bwd(args).  Computed by the plan the launchers dispatch on (csrc/gcn_b16.hip gcn_fwd_plan / gcn_bwd_plan), RECON_GCN_FUSED
 * and RECON_GCN_FUSED_BWD included; host arithmetic only: no device is needed and the pointers are looked at for null and for alignment,
 * never followed.  Returns -1 where the call would be refused, 0 where it launches nothing (B == 0, total_rows == 0), else
 *   forward   1  k_gcn_b16_fused_fwd<4, true>   (support == NULL; n % 4 == 0, out % 4 == 0, adj and bias 8-byte aligned: 8-byte loads)
 *             2  k_gcn_b16_fused_fwd<2, false>  (support == NULL; element loads of adj and bias)
 *             3  k_gemm_b16 + k_gcn_b16_aggregate (support given)
 *             4  the same over a ragged batch (node_ptr given)
 *   backward  path * 100000 + g_adj * 10000 + bias * 1000 + splits
 *             path    1 k_gcn_b16_fused_bwd (g_support and g_x in one launch), 2 k_gcn_b16_aggregate (+ k_gemm_b16 for g_x)
 *             g_adj   1 where k_gcn_b16_grad_adj is launched
 *             bias    0 no g_bias, 1 its second pass rides in k_b16_reduce behind the weight gradient, 2 k_gcn_b16_bias_reduce alone
 *             splits  split-K count of k_gemm_b16_kmajor for g_weight (1 .. 64), 0 without g_weight
 * e.g. 101017 = fused backward, g_bias in the reduce, 17 splits. */
int32_t recon_gcn_b16_fwd_instance(const recon_gcn_b16_args* args);
int32_t recon_gcn_b16_bwd_instance(const recon_gcn_b16_bwd_args* args);

/* L GraphConvolutions that share one adjacency (models/layers.py:57-63 applied L times, as the reference's stacks do), INFERENCE, in one
 * launch: the activations of a graph stay in LDS between the layers ("fused 3-hop, H resident in LDS").  Results are bit-equal
 * to L calls of recon_gcn_b16_fwd's fused form.  Layer 0: in_features -> hidden; layers 1 .. L-1: hidden -> hidden.  Shapes: n <= 32,
 * n % 4 == 0, hidden % 4 == 0, hidden <= 320, L <= 8, in_features <= 384 (L > 4: <= 352 — the activations of four graphs and the layers'
 * bias rows share the LDS); everything else answers RECON_ERR_UNSUPPORTED (the caller then runs layer by layer). */
typedef struct {
    int32_t B, n, in_features, hidden, L;
    const void* x; int64_t ldx;     /* [B*n, ldx] bf16, any even ldx >= in_features (the K tail is masked)                      */
    const void* adj;                /* [B, n, n] bf16, 8-byte aligned                                                          */
    const void* const* w_planes;    /* HOST array of L device pointers: W_l^T zero padded along k, [hidden][kp(in_l)] bf16,     *
                                     * written by recon_gcn_b16_transposed_planes() (kp = rounded up to 32)                     */
    const void* const* bias;        /* HOST array of L device pointers [hidden] bf16 (entries, or the array, may be NULL)       */
    void* out; int64_t ldo;         /* [B*n, ldo] bf16, ldo % 8 == 0; columns hidden .. ldo are written as zeros                */
} recon_gcn_b16_stack_args;
int recon_gcn_b16_stack_fwd(const recon_gcn_b16_stack_args* args, recon_stream_t stream);
/* The same stack WITH gradients (training; `gcn_layers.gcn_stack` under autograd): models/layers.py:57-63 applied L times + autograd.
 *   forward : one launch — the kernel above, which also keeps every layer's result (`acts`: the backward's ReLU masks and the operands of the
 *             weight gradients) — behind one repacking launch per layer (`planes`);
 *   backward: one launch for the whole chain g_support_l = adj^T (g_l . [act_l > 0]),  g_{l-1} = g_support_l W_l^T  (the gradient of a graph
 *             stays in LDS between the layers), then ONE k-major split-K launch for every layer's g_W_l = x_l^T g_support_l and one second
 *             pass that also finishes the g_bias_l.
 * Output, g_x and g_bias are bit-equal to L calls of recon_gcn_b16_fwd / recon_gcn_b16_bwd; g_W differs from theirs by the summation
 * order of the split-K partials only (fixed, run-to-run reproducible).  Shapes as for recon_gcn_b16_stack_fwd, and in_features <= 320. */
typedef struct {
    int32_t B, n, in_features, hidden, L;
    const void* x; int64_t ldx;         /* [B*n, ldx] bf16; ldx % 8 == 0 — or, with x_rows set, any even ldx >= in_features (read in place)     */
    void* x_rows; int64_t ldxr;         /* optional [B*n, ldxr] bf16, ldxr % 8 == 0: the forward leaves x here with 16-byte aligned rows for     *
                                         * layer 0's weight gradient (feature counts like 300: no repacking pass in front of the call)          */
    const void* adj;                    /* [B, n, n] bf16, 8-byte aligned                                                                      */
    const void* const* weight;          /* HOST array of L device pointers W_l [in_l][hidden] bf16, contiguous                                 */
    const void* const* bias;            /* HOST array of L device pointers [hidden] bf16 (entries, or the array, may be NULL)                  */
    void* const* planes;                /* HOST array of L workspaces of recon_gcn_b16_planes_bytes(in_l, hidden) bytes: written by the        *
                                         * forward, read by the backward                                                                      */
    void* const* acts; int64_t ldo;     /* HOST array of L buffers [B*n, ldo] bf16 (ldo % 8 == 0, ldo <= hidden rounded up to 32, else        *
                                         * RECON_ERR_UNSUPPORTED): the result of every layer, acts[L-1] = the stack's result; columns         *
                                         * hidden .. ldo are written as zeros                                                                 */
    /* ---- backward only ---- */
    const void* grad_out; int64_t ldg;  /* [B*n, ldg] bf16: gradient of acts[L-1]; any even ldg >= hidden, 4-byte aligned (read in place)      */
    void* const* g_support;             /* HOST array of L workspaces [B*n, ldo] bf16; columns hidden .. ldo are written as zeros              */
    float* partial;                     /* recon_gcn_b16_stack_bwd_partial_floats() floats                                                     */
    void* g_x; int64_t ldgx;            /* [B*n, ldgx] bf16 or NULL; ldgx % 4 == 0, >= in_features rounded up to 4, 8-byte aligned              */
    void* const* g_weight;              /* HOST array of L device pointers [in_l][hidden] bf16 (entries, or the array, may be NULL)            */
    void* const* g_bias;                /* HOST array of L device pointers [hidden] bf16 (entries, or the array, may be NULL)                  */
    const void* zeros;                  /* >= 1 KiB of zero bytes, 16-byte aligned                                                             */
} recon_gcn_b16_stack_train_args;
int recon_gcn_b16_stack_train_fwd(const recon_gcn_b16_stack_train_args* args, recon_stream_t stream);
size_t recon_gcn_b16_stack_bwd_partial_floats(int32_t B, int32_t n, int32_t in_features, int32_t hidden, int32_t L);
int recon_gcn_b16_stack_train_bwd(const recon_gcn_b16_stack_train_args* args, recon_stream_t stream);
/* planes [out_features][kp(in_features)] (bf16, (out_features * kp(in_features) * 2 bytes) of a weight [in_features][out_features] */
int recon_gcn_b16_transposed_planes(const void* weight, int32_t in_features, int32_t out_features, void* planes, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * K4  fp32 MFMA GEMM used by the projections, exported for tests:
 *     C[M,N] = A[M,K] * B (B given as [N,K] when b_is_nk != 0, else [K,N]); plain row-major.
 * ------------------------------------------------------------------------------------------*/
int recon_sgemm(int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, const float* B, int32_t ldb,
                int32_t b_is_nk, float* C, int32_t ldc, recon_stream_t stream);

/* The same kernels with the operands in three of the four orientations — A is [M,K] (a_is_km == 0) or [K,M]; B is [K,N] (b_is_nk == 0)
 * or [N,K]; A [K,M] together with B [N,K] has no kernel and answers RECON_ERR_UNSUPPORTED (nothing is written) —
 * and split-K (fixed-order second pass) when `workspace` (recon_sgemm_ex_workspace_floats() floats, may be 0) is given: what the
 * models' dense products outside the attention layer run on (`entity_embeddings.mm(self.W_entities)`, GAT/models.py:177, and the
 * gradients of it), in place of the library GEMM behind torch.mm.  Any lda / ldb / ldc and any base alignment: 16-byte loads and
 * stores are used where every stride, base and contiguous extent allows them, single floats otherwise. */
size_t recon_sgemm_ex_workspace_floats(int32_t M, int32_t N, int32_t K);
int recon_sgemm_ex(int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, int32_t a_is_km, const float* B, int32_t ldb,
                   int32_t b_is_nk, float* C, int32_t ldc, float* workspace, recon_stream_t stream);

/* Small dense products (tens of MFLOP), plain fp32 FMAs with K split 16 ways inside a workgroup and a fixed-order combine:
 *     C[M,N] = op(A) * op(B);  A is [M,K] (a_is_km == 0) or [K,M]; B is [K,N] (b_is_nk == 0) or [N,K].
 * Replaces `relation_embed.mm(self.W)` (GAT/models.py:75) and its two gradient products, which are launch / latency bound on tile GEMMs. */
size_t recon_sgemm_small_workspace_floats(int32_t M, int32_t N, int32_t K);  /* 0: no workspace needed */
/* workspace: recon_sgemm_small_workspace_floats() floats, or NULL.  With it, products with few output tiles and a long K (weight
 * gradients: 50 x 200 over K = 14 541 rows) also cut K over workgroups and add the parts in fixed order.  A leading dimension below
 * its operand's row length (lda < K resp. M, ldb < N resp. K, ldc < N): RECON_ERR_INVALID.  M == 0 or N == 0: RECON_OK, nothing is
 * launched.  K == 0: C's M x N elements are set to zero. */
int recon_sgemm_small(int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, int32_t a_is_km, const float* B, int32_t ldb,
                      int32_t b_is_nk, float* C, int32_t ldc, float* workspace, recon_stream_t stream);

/* K4'  the same product C[M,N] = A[M,K] * B[N,K]^T at fp32 accuracy on the bf16 matrix cores: every fp32
 * operand is split into three bfloat16 terms and six term products are accumulated in fp32
 * (csrc/gemm_bx3.hip).  B is split into `workspace` (recon_sgemm_bx3_workspace_bytes) first; A on the fly.
 * Requires K % 4 == 0 and 16-byte aligned A rows (RECON_ERR_UNSUPPORTED otherwise).  Exported for tests;
 * the GAT layer uses it for the projection `self.a.mm(...)` (GAT/layers.py:129-137) and its input gradient. */
size_t recon_sgemm_bx3_workspace_bytes(int32_t N, int32_t K);
int recon_sgemm_bx3(int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, const float* B, int32_t ldb,
                    float* C, int32_t ldc, void* workspace, recon_stream_t stream);
/* C[M,N] = A^T * B for k-major operands A[K,M], B[K,N] (the weight-gradient form g_a^T = V^T g_h; split-K with a
 * fixed-order second pass; A is split on the fly, B into `workspace` first).  Requires M and lda to be multiples
 * of 4 (RECON_ERR_UNSUPPORTED otherwise). */
size_t recon_sgemm_bx3_tn_workspace_bytes(int32_t M, int32_t N, int32_t K);
int recon_sgemm_bx3_tn(int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, const float* B, int32_t ldb,
                       float* C, int32_t ldc, void* workspace, recon_stream_t stream);

/* K4''  the same two products on the fp16 matrix cores with TWO half terms per operand and three term products
 * (csrc/gemm_hx2.hip): every operand is scaled by a per-tensor power of two taken from its max magnitude, so that
 * half's 5 exponent bits suffice, and pre-split into two half planes; fp32-class accuracy at half the MFMA work of
 * the bf16 x 3 form.  These stand-alone entries measure (amax) and split both operands into `workspace` (256-byte
 * aligned) first; the *_presplit forms re-run only the GEMM on the planes a previous call left there (benchmarks).
 * Requires K % 8 == 0 (k-contiguous form; RECON_ERR_UNSUPPORTED otherwise); any M, N for the k-major form.  A workspace that is not
 * 256-byte aligned is an argument error (RECON_ERR_INVALID), like a null one.  In the GAT layer the planes are written by
 * the kernels that produce the operands (edge aggregation: V; ELU-gradient pass: g_h). */
size_t recon_hx2_aux_bytes(void);      /* size of recon_gat_atp_args.aux */
size_t recon_sgemm_hx2_workspace_bytes(int32_t M, int32_t N, int32_t K);
int recon_sgemm_hx2(int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, const float* B, int32_t ldb,
                    float* C, int32_t ldc, void* workspace, recon_stream_t stream);
int recon_sgemm_hx2_presplit(int32_t M, int32_t N, int32_t K, float* C, int32_t ldc, void* workspace, recon_stream_t stream);
size_t recon_sgemm_hx2_tn_workspace_bytes(int32_t M, int32_t N, int32_t K);
int recon_sgemm_hx2_tn(int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, const float* B, int32_t ldb,
                       float* C, int32_t ldc, void* workspace, recon_stream_t stream);
int recon_sgemm_hx2_tn_presplit(int32_t M, int32_t N, int32_t K, float* C, int32_t ldc, void* workspace, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * N1  the stage-A loop's loss: batch_gat_loss, GAT/main.py:344-376, with gat_loss_func = nn.MarginRankingLoss(margin) (mean reduction):
 *     triples int64 [n_pos (1 + reps)][3] = (head, relation, tail): n_pos positives, then reps corrupted copies of the block
 *     (reps = 2 * valid_invalid_ratio_gat); pair j compares positive j % n_pos with negative j:
 *     loss = mean_j max(0, |e[h] + r[rel] - e[t]|_1 (positive) - |...|_1 (negative) + margin).
 * fwd (two launches): terms [pairs], loss [1]; ent_key int64 [2][4 pairs] / rel_key int64 [2][2 pairs] (optional) receive the table row of every
 * gradient row the backward writes — the segment keys of recon_spmm_rowsum_fwd (row 0 = key, row 1 = copy).  `counter`: unused (may be NULL);
 * one workgroup adds the terms in index order.
 * bwd: g_ent_rows [4 pairs][D] (positive heads | positive tails | negative heads | negative tails), g_rel_rows [2 pairs][D]
 * (positive | negative); the tables' gradients are their sums by key.  Ids are not range-checked (the caller validates, as for edges). */
int recon_transe_margin_fwd(const float* entity, const float* relation, const int64_t* triples, int64_t n_pos, int32_t reps, int32_t D,
                            float margin, float* terms, float* loss, int64_t* ent_key, int64_t* rel_key, uint32_t* counter,
                            recon_stream_t stream);
/* recon_transe_margin_fwd with ONE key tensor for both tables: keys int64 [2][6 P] (P = n_pos * reps) — the four entity ids of pair j at
 * [q P + j], q < 4, its two relation ids PLUS n_entities at [4 P + q P + j], q < 2 (second row: a copy).  The backward's gradient rows, written
 * as one [6 P, D] block (g_ent_rows = block, g_rel_rows = block + 4 P D), are then summed into a [n_entities + n_relations, D] table by ONE
 * destination-only graph build and ONE recon_spmm_rowsum_fwd instead of two of each. */
int recon_transe_margin_fwd_keys(const float* entity, const float* relation, const int64_t* triples, int64_t n_pos, int32_t reps, int32_t D,
                                 float margin, float* terms, float* loss, int64_t* keys, int64_t n_entities, recon_stream_t stream);
int recon_transe_margin_bwd(const float* entity, const float* relation, const int64_t* triples, int64_t n_pos, int32_t reps, int32_t D,
                            const float* terms, const float* g_loss, float* g_ent_rows, float* g_rel_rows, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * N1  the stage-A batch builders on the device: Corpus.get_batch_adj_data (GAT/create_batch.py:391-436) and
 * Corpus.get_batch_nhop_neighbors_all (:871-895) over the 2-hop neighbourhoods that Corpus.bfs / get_further_neighbors (:788-869) precompute
 * on the host.  The knowledge graph is the grouped CSR recon_amd.sampler.KGNeighbourSampler builds once: (source, target) pairs grouped
 * by source in order of first appearance, the relations of a pair contiguous in insertion order.  All ids int64, device memory.
 *
 * recon_kg_adj_count: per batch position its number of edges nrel [B]; the LAST workgroup scans them (rel_off [B], totals[0] = E) and
 *   compacts the marks into the sorted unique entity / target id lists (uniq_ent, uniq_tgt: room for num_entities ids; totals[1], totals[2]
 *   = their lengths).  ent_mark / tgt_mark: num_entities zeroed bytes each, handed back zeroed; counter: one zeroed uint32, handed back zero.
 * recon_kg_adj_fill: edge int64 [2][E] (row 0 targets, row 1 sources) and edge_type [E], after the caller has read E.
 * recon_kg_nhop: write = 0 counts the quadruples of every source (qcount [S], quad_off [S], total[0]), write = 1 writes them
 *   (quads int64 [total][4] = source, first relation source -> parent, first relation parent -> target, target) in BFS discovery order.
 *   One wave per source, its visited set as a bitmap in LDS (recon_kg_nhop_lds_bytes; RECON_ERR_UNSUPPORTED beyond a CU's LDS). */
typedef struct recon_kg {
    int64_t num_entities;
    const int64_t* pair_ptr;        /* [num_entities + 1] pairs of source s: [pair_ptr[s], pair_ptr[s + 1]) */
    const int64_t* pair_tgt;        /* [P] */
    const int64_t* pair_first_rel;  /* [P] first relation of the pair */
    const uint8_t* not_loop;        /* [P] 0 for (s, s) pairs */
    const int64_t* rel_ptr;         /* [P + 1] relations of pair p: [rel_ptr[p], rel_ptr[p + 1]) */
    const int64_t* rel_sorted;      /* [T] */
} recon_kg;
size_t recon_kg_nhop_lds_bytes(int64_t num_entities);
int recon_kg_adj_count(const recon_kg* kg, const int64_t* entities, int32_t B, int64_t* nrel, uint8_t* ent_mark, uint8_t* tgt_mark,
                       int64_t* rel_off, int64_t* uniq_ent, int64_t* uniq_tgt, int64_t* totals, uint32_t* counter, recon_stream_t stream);
int recon_kg_adj_fill(const recon_kg* kg, const int64_t* entities, int32_t B, const int64_t* rel_off, int64_t E, int64_t* edge,
                      int64_t* edge_type, recon_stream_t stream);
int recon_kg_nhop(const recon_kg* kg, const int64_t* sources, int32_t S, int32_t partial_2hop, int32_t write, int64_t* qcount, int64_t* quad_off,
                  int64_t* quads, int64_t* total, uint32_t* counter, recon_stream_t stream);
/* recon_kg_nhop's count pass (write = 0) over a source list whose LENGTH is still on the device: sources has room for S_max ids, *s_dev of them are
 * valid (the unique-entity list and its count as recon_kg_adj_count leaves them).  Queued behind recon_kg_adj_count, it lets the caller read the
 * 1-hop sizes and the 2-hop total in one host round trip; the write pass is recon_kg_nhop(write = 1) with the count the host then knows. */
int recon_kg_nhop_count_early(const recon_kg* kg, const int64_t* sources, int32_t S_max, const int64_t* s_dev, int32_t partial_2hop, int64_t* qcount,
                              int64_t* quad_off, int64_t* total, recon_stream_t stream);
/* Dead-row pruning of a batch graph for SpKBGATModified (GAT/models.py:167-178: the model keeps `mask * out_entity_1`, so an edge matters only
 * if its destination lies in need = mask U { src(e) : mask[dst(e)] != 0 }).  edge int64 [2][E1] (row 0 destinations) with type [E1], edge_nhop
 * [2][E2] with type_nhop [E2][2] (E2 = 0: none); mask float [N]; need: N bytes of scratch.  The surviving edges are written in their
 * input order: out_edge (room for [2][E1]) holds the destinations at [0, counts[0]) and the sources at [E1, E1 + counts[0]) — the caller's
 * [2, counts[0]] tensor is a view with row stride E1 —, out_type [counts[0]]; likewise out_edge_nhop (row stride E2), out_type_nhop
 * [counts[1]][2].  pos (optional, E1 + E2): the survivors' positions in the concatenated input, the 1-hop ones at [0, counts[0]), the n-hop ones
 * (values from E1) at [E1, E1 + counts[1]).  counts: device int64 [2], read by the caller (one synchronisation).  One launch of one workgroup:
 * batch graphs are tens of thousands of edges. */
int recon_edges_prune(const int64_t* edge, const int64_t* type, int64_t E1, const int64_t* edge_nhop, const int64_t* type_nhop, int64_t E2,
                      const float* mask, int32_t N, uint8_t* need, int64_t* out_edge, int64_t* out_type, int64_t* out_edge_nhop,
                      int64_t* out_type_nhop, int64_t* pos, int64_t* counts, recon_stream_t stream);
/* The same for a whole SpKBGATModified call (GAT/models.py:136-178), one launch: mask [N] is MADE here (zeros, 1.0 at batch_entities [B]; an id
 * outside [0, N) sets counts[2]: the reference's indexing raises), the n-hop list arrives as the quadruples [E2][4] = (source, rel_1, rel_2,
 * target) it is derived from (:145-148), and the survivors of both lists go into ONE buffer out_edge [2][E1 + E2] (row stride E1 + E2), the
 * 1-hop ones at [0, counts[0]), the n-hop ones at [counts[0], counts[0] + counts[1]): the caller's 1-hop, n-hop and concatenated edge tensors are
 * views of it.  out_type [E1], out_type_nhop [E2][2], pos as above; counts: device int64 [3]. */
int recon_edges_prune_batch(const int64_t* batch_entities, int32_t B, const int64_t* edge, const int64_t* type, int64_t E1, const int64_t* quads,
                            int64_t E2, int32_t N, float* mask, uint8_t* need, int64_t* out_edge, int64_t* out_type, int64_t* out_type_nhop,
                            int64_t* pos, int64_t* counts, int64_t* ext_index /* optional, E1 + E2 */, int64_t ext_base, recon_stream_t stream);
/* ext_index: the row of the layers' edge-embedding table each surviving edge reads (GAT/layers.py:126-127 with `relation_embed[edge_type]` read in
 * place): a 1-hop edge its relation id, the j-th surviving n-hop edge row ext_base + j (ext_base = rows of the relation table). */
/* CSR-slot order of an index tensor in one launch: out32[k] = out64[k] = index[eid[k]] (recon_gat_atp_args.ee_index and the segment key of the
 * table gradient). */
int recon_slot_index(const int64_t* index, const int32_t* eid, int32_t E, int32_t* out32, int64_t* out64, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * N1  the tail of SpKBGATModified (GAT/models.py:167-180) and the row normalisation of the entity table (:160):
 *     y[r] = t / max(|t|_2, eps),  t = ew[r] + mask[r] * skip[r]        (skip, mask may be NULL: plain F.normalize(ew, p=2, dim=1); y may alias ew)
 * norm [N] (optional) receives |t|_2 for the backward:  g_t = (g_y - y (y . g_y)) / |t|  (g_y / eps below the clamp), g_skip = mask * g_t. */
int recon_rows_normalize_fwd(const float* ew, const float* skip, const float* mask, int64_t N, int32_t C, float eps, float* y, float* norm,
                             recon_stream_t stream);
int recon_rows_normalize_bwd(const float* g_y, const float* y, const float* norm, const float* mask, int64_t N, int32_t C, float eps, float* g_t,
                             float* g_skip, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * E1  link-prediction evaluation of the ConvKB scorer (csrc/kg_eval.hip): SpKBGATConvOnly.batch_test (GAT/models.py:300-304) ->
 *     ConvKB.forward (GAT/layers.py:41-46) over every candidate of one slot of every test triple, as Corpus.get_validation_pred
 *     (GAT/create_batch.py:905-1099) and get_validation_cnfmat (:1365-1420) run it.  fc1 is split along its concatenated input:
 *     P_h = E W_h^T, P_r = Rel W_r^T, P_t = E W_t^T (W1 = [W_h | W_r | W_t], recon_sgemm_ex with ldb = 3 D), and
 *         s(q, c) = b2 + sum_d w2[d] leaky(u[q, d] + P_slot[c, d]),   u[q] = (P_a[a] + P_b[b]) + b1,   leaky(x) = max(x, slope x)
 *     with (a, b) the two other columns of the triple in column order.  slot = the column replaced: 0 head, 1 relation, 2 tail.
 *     triples int64 [Q][3] = (head, relation, tail); P_h, P_t [n_ent][D], P_r [n_rel][D]; b1, w2 [D]; b2 [1] (device, read by the kernels);
 *     0 <= slope <= 1 (RECON_ERR_UNSUPPORTED otherwise; the reference's nl1 = nn.LeakyReLU(): 0.01).  Every score comes from ONE routine with
 *     one summation order, so a (query, candidate) scores bit-identically in both entry points.  Ids are range-checked by the caller
 *     (recon_amd.kg_eval); the kernels never read outside a table: a query with an id outside its table gets rank 0 and a NaN score (a NaN
 *     dense score), an excluded id outside the candidate table is ignored.
 * ------------------------------------------------------------------------------------------*/
enum { RECON_KGE_HEAD = 0, RECON_KGE_RELATION = 1, RECON_KGE_TAIL = 2 };
/* Filtered rank without the Q x N score matrix (:934-1020): ranks int64 [Q] = 1 + #{c not excluded : s(q, c) > s*(q)}, true_scores [Q] = s*(q)
 * = s(q, true id).  That is the position of the true triple in a stable descending sort with the true triple inserted at index 0 (:965-968,
 * :1016-1020): ties count for the true triple.  The excluded ids of query q are filt_ids[filt_begin[q] .. filt_end[q]) (int64, no duplicates;
 * may contain the true id; filt_ids NULL: raw ranks) — valid_triples_dict's members among the candidates (:947-963).  workspace:
 * recon_convkb_rank_workspace_floats(Q, D) floats.  Two launches; the rank is an integer sum, deterministic. */
size_t recon_convkb_rank_workspace_floats(int64_t Q, int32_t D);
int recon_convkb_rank(int32_t slot, int64_t Q, const int64_t* triples, const float* P_h, const float* P_r, const float* P_t, int64_t n_ent,
                      int64_t n_rel, int32_t D, const float* b1, const float* w2, const float* b2, float slope, const int64_t* filt_ids,
                      const int64_t* filt_begin, const int64_t* filt_end, float* workspace, size_t workspace_floats, int64_t* ranks,
                      float* true_scores, recon_stream_t stream);
/* Dense scores S[q][j] = s(q, c0 + j), j < C, row stride ldS >= C: with slot = RECON_KGE_RELATION and [c0, c0 + C) = [0, n_rel) the `scores`
 * tensor of get_validation_cnfmat (:1369-1420) laid out [Q][n_rel].  Q <= 65535 per call. */
int recon_convkb_scores(int32_t slot, int64_t Q, const int64_t* triples, const float* P_h, const float* P_r, const float* P_t, int64_t n_ent,
                        int64_t n_rel, int32_t D, const float* b1, const float* w2, const float* b2, float slope, int64_t c0, int64_t C, float* S,
                        int64_t ldS, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * E3  link-prediction evaluation of the GAT_sep_space ConvKB scorer (csrc/kg_sep.hip, csrc/kg_eval.hip): SpKBGATConvOnly.batch_test
 *     (GAT_sep_space/models.py:316-339) carries both entities into the triple's relation space, e' = tanh(E[e] W_ent2rel[r]), before ConvKB.
 *     Corpus.get_validation_cnfmat (GAT_sep_space/create_batch.py:1360-1390) scores every test triple with every relation through it, 100
 *     rows and a [100, D, D] gather of W_ent2rel per call; get_validation_pred (:905-1199) cannot run it (batch_test takes model_gat).
 *     With W1 = [W_h | W_r | W_t] the entity tables of E1 become per relation: P_h^r = tanh(E W_ent2rel[r]) W_h^T, P_t^r = tanh(E W_ent2rel[r])
 *     W_t^T; P_r = Rel W_r^T is E1's.  A chunk of Rc relations rel_ids (int64, device) has tables P_h, P_t [Rc][n][D] (local relation rl at
 *     offset rl n D), and every score is E1's routine on the tables of the query's relation: bit-identical to recon_convkb_rank /
 *     recon_convkb_scores run on ONE relation's tables.
 * ------------------------------------------------------------------------------------------*/
/* The tables of a relation chunk (the tanh(bmm(e, W_ent2rel[r])) of :316-320 and the entity part of fc1, GAT_sep_space/layers.py ConvKB):
 * row m of local relation rl is built from E[ids[m]] (ids int64 [U], device; NULL: row m of E, U <= n_rows).  E [n_rows][D], W_ent2rel
 * [n_rel][D][D] laid out [in][out] (x . W), W1 = fc1.weight [D][3 D] read in place.  1 <= D <= 512, Rc <= 65535.  Exact fp32 products
 * (v_mfma_f32_16x16x4_f32), tanh in fp32; tanh(E_tile W_r) stays in LDS.  A relation id outside [0, n_rel) gives NaN tables; an entity id
 * outside [0, n_rows) gives the row of a zero entity.  No atomics: bitwise identical from run to run.  One launch. */
int recon_kgsep_tables(const float* E, int64_t n_rows, const int64_t* ids, int64_t U, const float* W_ent2rel, int64_t n_rel, const int64_t* rel_ids,
                       int32_t Rc, const float* W1, int32_t D, float* P_h, float* P_t, recon_stream_t stream);
/* The rows the training step of the sep scorer feeds ConvKB (SpKBGATConvOnly.forward, GAT_sep_space/models.py:311-324: the [M, D, D] gather
 * W_ent2rel[batch[:, 1]], two bmm and tanh of :312-320): T [2 M][D] fp32 with T[m] = tanh(E[h_m] W_ent2rel[r_m]) and T[M + m] =
 * tanh(E[t_m] W_ent2rel[r_m]), and remapped int64 [M][3] = (m, r_m, M + m), so that recon_convkb_train_fwd / _bwd score the batch with
 * E := T, n_ent := 2 M.  triples int32 or int64 [M][3] (index_bytes 4 or 8), E [n_ent][D], W_ent2rel [n_rel][D][D] laid out [in][out].
 * Item i < M is the head of triple i, item M + i its tail; order int64 [2 M] holds the items sorted by relation and seg int64 [n_rel + 1]
 * delimits relation r's items, order[seg[r] .. seg[r + 1]) (device, no host read: a stable argsort and a bincount / cumsum of the relation
 * column, with ids outside [0, n_rel) clamped into it first).  An item whose entity id lies outside [0, n_ent) or whose relation is not
 * the one it was sorted under gets a NaN row, so the triple scores NaN.  Exact fp32 products (v_mfma_f32_16x16x4_f32), tanh in fp32; one
 * lane writes each element, no atomics: bitwise identical from run to run.  1 <= D <= 512 (RECON_ERR_UNSUPPORTED above), M < 2^31.
 * One launch of ceil(2 M / (16 RB)) + n_rel workgroups; those without a tile leave at once. */
int recon_kgsep_ent2rel(const void* triples, int32_t index_bytes, int64_t M, const float* E, int64_t n_ent, const float* W_ent2rel, int64_t n_rel,
                        int32_t D, const int64_t* order, const int64_t* seg, float* T, int64_t* remapped, recon_stream_t stream);
/* Filtered (or raw) head or tail ranks (slot RECON_KGE_HEAD / RECON_KGE_TAIL) of queries sorted by relation, on one chunk's tables
 * (n_ent = rows per relation): the queries of local relation rl are triples[seg[rl] .. seg[rl + 1]) (seg int64 [Rc + 1], device,
 * non-decreasing, seg[0] = 0, seg[Rc] = Q), their relation column is rel_ids[rl] (it indexes P_r).  Ranks, true scores, the filter and the
 * workspace (recon_convkb_rank_workspace_floats(Q, D) floats) as recon_convkb_rank, with the same tie rule and integer count.  64-query tiles
 * never cross a relation; two launches per chunk and side, none per relation, no host read. */
int recon_kgsep_rank(int32_t slot, int64_t Q, const int64_t* triples, const int64_t* seg, int32_t Rc, const float* P_h, const float* P_r,
                     const float* P_t, int64_t n_ent, int64_t n_rel, int32_t D, const float* b1, const float* w2, const float* b2, float slope,
                     const int64_t* filt_ids, const int64_t* filt_begin, const int64_t* filt_end, float* workspace, size_t workspace_floats,
                     int64_t* ranks, float* true_scores, recon_stream_t stream);
/* Relation scores of the sep scorer, the `scores` of :1360-1390 laid out [Q][n_rel] (before its view(-1, num_rels)): S[q][rel_ids[rl]] = the
 * score of triple q with relation rel_ids[rl], its head and tail rows (triples' columns 0 and 2, rows of the chunk's tables) read from local
 * relation rl's tables; u = (P_h^r' + P_t^r') + b1, candidate P_r[r'].  Other columns of S are not written; ldS >= n_rel. */
int recon_kgsep_scores(int64_t Q, const int64_t* triples, const int64_t* rel_ids, int32_t Rc, const float* P_h, const float* P_r, const float* P_t,
                       int64_t n_ent, int64_t n_rel, int32_t D, const float* b1, const float* w2, const float* b2, float slope, float* S, int64_t ldS,
                       recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * E4  the stage-A translation loss of the GAT_sep_space tree (csrc/kg_sep.hip): batch_gat_loss, GAT_sep_space/main.py:347-391, with
 *     gat_loss_func = nn.MarginRankingLoss(margin) (mean reduction).  triples int64 [M][3], M = n_pos (1 + reps): the positives, then reps
 *     corrupted copies of the block (reps = 2 * valid_invalid_ratio_gat).  T [2 M][D] = recon_kgsep_ent2rel's rows of the batch, every
 *     triple carried into its relation's space ONCE (the reference tiles the positives reps times first); Rel [n_relp][D].
 *         x_i = (T[i] + Rel[r_i]) - T[M + i],  norm_i = |x_i|_1,  term_j = max(0, norm_{j mod n_pos} - norm_{n_pos + j} + margin), j < P = n_pos reps,
 *         loss = mean_j term_j  (a NaN norm reaches its terms and the loss, and raises the device's NaN word, as recon_transe_margin_fwd does).
 * ------------------------------------------------------------------------------------------*/
/* Forward: norms [M], terms [P], loss [1].  Two launches; every sum has one order.  A relation id outside [0, n_relp) gives a NaN norm. */
int recon_kgsep_gat_loss_fwd(const int64_t* triples, int64_t n_pos, int32_t reps, const float* T, const float* Rel, int64_t n_relp, int32_t D,
                             float margin, float* norms, float* terms, float* loss, recon_stream_t stream);
/* Backward through the norms, the relation-space map and tanh, from the upstream scalar g_loss [1] (device) and the forward's T and terms:
 *     c_i = +(g / P) #{k : term_{k n_pos + i} > 0} (positive i), -(g / P) [term_{i - n_pos} > 0] (negative i),  gx_i = c_i sign(x_i), sign(0) = 0,
 *     gpre[i] = gx_i (1 - T[i]^2),  gpre[M + i] = -gx_i (1 - T[M + i]^2),
 *     g_rows [2 M][D]:       g_rows[item] = gpre[item] W_ent2rel[r]^T  (the caller sums them by entity id into the entity table's gradient),
 *     g_W    [n_rel][D][D]:  g_W[r] = sum over the items of relation r of E[e_item]^T gpre[item]  (zeros for a relation without items),
 *     g_Rel  [n_relp][D]:    g_Rel[r] = sum over the triples of relation r of gx_i; rows r >= n_rel are NOT written.
 * A pair is active where its term is > 0 (torch's clamp_min backward also passes a pre-clamp value of exactly 0: the two differ only there).
 * Each of the three may be NULL: its work is skipped.  order / seg: the relation-ordered walk recon_kgsep_ent2rel took.  gpre is formed
 * on the fly; both products run on v_mfma_f32_16x16x4_f32 in fp32.  Every output element is one k-ordered chain over the walk, written
 * once by one lane: no partial sums across workgroups, no arrival counters, no atomics, bitwise identical from run to run.  An item with
 * an id outside its table gets a NaN row of g_rows and adds nothing to g_W / g_Rel.  1 <= D <= 512 (RECON_ERR_UNSUPPORTED above).
 * workspace: recon_kgsep_gat_loss_bwd_workspace_bytes(M) bytes, 8-byte aligned, any contents.  Up to three launches. */
size_t recon_kgsep_gat_loss_bwd_workspace_bytes(int64_t M);
int recon_kgsep_gat_loss_bwd(const int64_t* triples, int64_t n_pos, int32_t reps, const float* E, int64_t n_ent, const float* Rel, int64_t n_relp,
                             const float* W_ent2rel, int64_t n_rel, int32_t D, const int64_t* order, const int64_t* seg, const float* T,
                             const float* terms, const float* g_loss, void* workspace, size_t workspace_bytes, float* g_rows, float* g_W,
                             float* g_Rel, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * E5  RECON's per-relation translation residuals (csrc/rel_trans.hip): models/models.py:939-958,
 *         out[m][r] = sum_d | tanh(head_m . W_r)_d + rel[r][d] - tanh(tail_m . W_r)_d |,
 *     head, tail [M][ent_dim] with row strides ld_head, ld_tail in elements (the two halves of one [M][2 ent_dim] tensor are read in place),
 *     W [n_rel][ent_dim][rel_dim], rel [n_rel][rel_dim], out [M][n_rel], all fp32.  No [M][n_rel][rel_dim] tensor is written.
 * ------------------------------------------------------------------------------------------*/
/* Shapes the kernels take (models/models.py:939-958): 1 <= M <= 2^30, 1 <= n_rel <= 65535, 1 <= ent_dim <= 2^20, 1 <= rel_dim <= 256. */
int recon_rel_translation_supported(int64_t M, int32_t n_rel, int32_t ent_dim, int32_t rel_dim);
/* Bytes of the buffer the forward leaves for the backward (models/models.py:939-958): sgn of every difference as two bit planes, 2 words
 * per (relation, pair, 32 columns), 1/16 of an fp32 intermediate at rel_dim % 32 == 0.  8-byte aligned, any contents. */
size_t recon_rel_translation_saved_bytes(int64_t M, int32_t n_rel, int32_t rel_dim);
/* Forward (models/models.py:939-958).  Both products of a (64-pair tile, relation) run in one workgroup on v_mfma_f32_32x32x2_f32 (exact
 * fp32 fma chains, k ascending); tanh, + rel, -, |.| and the sum over rel_dim are the epilogue on the accumulators.  Every sum has one
 * order and one lane writes each element: bitwise identical from run to run.  saved: recon_rel_translation_saved_bytes() bytes, or NULL
 * when no backward follows.  Row strides above 2^22 elements: RECON_ERR_UNSUPPORTED.  M == 0: nothing is launched.  One launch. */
int recon_rel_translation_fwd(const float* head, int64_t ld_head, const float* tail, int64_t ld_tail, const float* W, const float* rel, int64_t M,
                              int32_t n_rel, int32_t ent_dim, int32_t rel_dim, float* out, void* saved, recon_stream_t stream);
/* Backward for rel (models/models.py:939-958): g_rel[r][d] = sum_m g_out[m][r] sgn(diff[m][r][d]) with sgn(0) = 0, from the forward's
 * `saved`; g_out [M][n_rel] contiguous.  Fixed order over m, no atomics: bitwise identical from run to run.  M == 0 writes zeros.
 * One launch. */
int recon_rel_translation_bwd(const float* g_out, const void* saved, int64_t M, int32_t n_rel, int32_t rel_dim, float* g_rel,
                              recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * E7  The entity-context encoder's character CNN (csrc/char_cnn.hip): models/models.py:57-61,
 *         pre[s][t][o] = conv_b[o] + sum_k sum_c emb[chars[s][t + k]][c] conv_w[o][c][k],
 *         out[s][w][o] = tanh(max over t in [w span, (w + 1) span) of pre[s][t][o]),
 *     chars [S][cfs - 1 + W span] int32 or int64 (index_bytes = 4 or 8; row stride ld_chars in elements, read in place), emb [V][C],
 *     conv_w [Fo][C][cfs], conv_b [Fo], out [S][W][Fo], all fp32 and contiguous.  No [S][Lc][.] tensor is written: the convolution of
 *     an embedding is cfs table lookups, T[k] = emb . conv_w[:, :, k]^T.  Ids outside [0, V) are clamped into the table.
 * ------------------------------------------------------------------------------------------*/
/* Shapes the kernels take (models/models.py:57-61): S, W, C >= 1, 1 <= span <= 255, 1 <= cfs <= 16, span + cfs - 1 <= 64 (one lane per
 * id of a word), 1 <= Fo <= 256, cfs V Fo <= 2^22, S W Fo <= 2^40. */
int recon_char_features_supported(int64_t S, int32_t W, int32_t span, int32_t cfs, int32_t V, int32_t C, int32_t Fo);
/* Bytes of the workspace (models/models.py:57-61) of the forward (backward = 0: the cfs tables) or of the backward (backward = 1: one
 * private dT [cfs][V][Fo] + d_bias [Fo] per workgroup, at most 512 of them, and their sum).  16-byte aligned, any contents; 0 for a
 * shape recon_char_features_supported refuses. */
size_t recon_char_features_workspace_bytes(int64_t S, int32_t W, int32_t span, int32_t cfs, int32_t V, int32_t C, int32_t Fo, int32_t backward);
/* Forward (models/models.py:57-61).  One wave per word, lane = output channel; the tables lie in LDS up to 144 KiB and are read through
 * L2 above.  The FIRST maximum of a window wins, as torch's max_pool1d picks it; arg_pos [S][W][Fo] (one byte each, or NULL when no
 * backward follows) receives its position in the window.  keep (dropout factors [S][Lc][C]) must be NULL, RECON_ERR_UNSUPPORTED otherwise:
 * the masked form takes packed bits (recon_char_masked_fwd).  S == 0: nothing is launched.  Two launches (tables, words). */
int recon_char_features_fwd(const void* chars, int32_t index_bytes, int64_t ld_chars, const float* emb, const float* conv_w, const float* conv_b,
                            const float* keep, int64_t S, int32_t W, int32_t span, int32_t cfs, int32_t V, int32_t C, int32_t Fo, float* out,
                            uint8_t* arg_pos, void* workspace, size_t workspace_bytes, recon_stream_t stream);
/* Backward (models/models.py:57-61) from the forward's out and arg_pos: d_pre = g_out (1 - out^2) goes to dT[k][chars[t* + k]][o] and to
 * g_conv_b; g_emb = sum_k dT[k] . conv_w[:, :, k] with row padding_idx zero (nn.Embedding's padding_idx; < 0: none), g_conv_w[:, :, k] =
 * dT[k]^T . emb.  g_out [S][W][Fo] contiguous.  No floating-point atomics: every workgroup owns a fixed run of words and a private dT
 * with one writer per cell, the workgroups are added in index order: bitwise identical from run to run.  keep must be NULL.  S == 0
 * writes zeros.  Three launches (and one memset when the private dT does not fit in LDS). */
int recon_char_features_bwd(const void* chars, int32_t index_bytes, int64_t ld_chars, const float* emb, const float* conv_w, const float* keep,
                            const float* g_out, const float* out, const uint8_t* arg_pos, int64_t S, int32_t W, int32_t span, int32_t cfs,
                            int32_t V, int32_t C, int32_t Fo, int32_t padding_idx, float* g_emb, float* g_conv_w, float* g_conv_b, void* workspace,
                            size_t workspace_bytes, recon_stream_t stream);

/* The same char-CNN WITH dropout factors on the gathered embedding (csrc/char_mask.hip; models/models.py:57-61 in training mode), the
 * factors packed: bits [S][Lc][KW] int32, KW = ceil(C / 32), Lc = cfs - 1 + W span, contiguous; factor (s, j, c) = scale if bit c % 32 of
 * word c / 32 is set, else 0.  Bits at and above C in the last word are ignored.
 *         X[j][c] = bit(s, j, c) ? emb[chars[s][j]][c] : 0,   pre[s][t][o] = conv_b[o] + scale sum_k sum_c X[t + k][c] conv_w[o][c][k].
 * A real fp32 convolution (v_mfma_f32_16x16x4_f32: an fp32 fma chain, no reduced-precision operand); nothing of size S Lc C is written.
 * Status codes, ids (int32 / int64, read in place through ld_chars, clamped into [0, V)) and the 16-byte workspace alignment are the
 * table form's. */
/* Shapes the masked kernels take (models/models.py:57-61): the table form's limits (S, W >= 1, 1 <= span <= 255, 1 <= cfs <= 16,
 * span + cfs - 1 <= 64, 1 <= Fo <= 256, S W Fo <= 2^40) and 1 <= C <= 64 (one lane per embedding channel in the backward, KW <= 2),
 * V C + Fo C cfs + Fo <= 2^22 (one private accumulator set of the backward). */
int recon_char_masked_supported(int64_t S, int32_t W, int32_t span, int32_t cfs, int32_t V, int32_t C, int32_t Fo);
/* Bytes of the workspace (models/models.py:57-61) of the masked forward (backward = 0: the filter bank as the MFMA's B operand) or
 * backward (backward = 1: one private dE [V][C] + dW [Fo][cfs][C] + db [Fo] per workgroup, at most 256 of them).  16-byte aligned, any
 * contents; 0 for a shape recon_char_masked_supported refuses. */
size_t recon_char_masked_workspace_bytes(int64_t S, int32_t W, int32_t span, int32_t cfs, int32_t V, int32_t C, int32_t Fo, int32_t backward);
/* Draws the bits of n_positions = S Lc character positions (the dropout of models/models.py:57-61 as packed bits) into bits
 * [n_positions][ceil(C / 32)].  Philox4x32-10 with key (low, high half of seed); position q owns the Gp = ceil(C / 4) counters
 * offset + q Gp + g (a 64-bit value: counter words 0 and 1, words 2 and 3 zero); channel c takes output word c % 4 of counter g = c / 4
 * and its bit is set iff word >= threshold, threshold = min(2^32 - 1, floor(p 2^32)) for a drop probability p.  Bits at and above C are
 * written as 0.  1 <= C <= 2^16.  One launch; n_positions == 0: none. */
int recon_char_keep_bits_draw(int32_t* bits, int64_t n_positions, int32_t C, uint32_t threshold_u32, uint64_t seed_u64, uint64_t offset_u64,
                              recon_stream_t stream);
/* Masked forward (models/models.py:57-61).  One wave per word: the word's masked rows are staged in LDS once and multiplied with the
 * filter bank on the fp32 MFMA; emb and the filter bank lie in LDS up to 144 KiB and are read through L2 above.  The FIRST maximum of a
 * window wins; a window whose taps are all masked or padding gives exactly tanh(conv_b[o]).  arg_pos as in recon_char_features_fwd
 * (NULL when no backward follows).  S == 0: nothing is launched.  Two launches (operand layout, words). */
int recon_char_masked_fwd(const void* chars, int32_t index_bytes, int64_t ld_chars, const float* emb, const float* conv_w, const float* conv_b,
                          const int32_t* bits, float scale, int64_t S, int32_t W, int32_t span, int32_t cfs, int32_t V, int32_t C, int32_t Fo,
                          float* out, uint8_t* arg_pos, void* workspace, size_t workspace_bytes, recon_stream_t stream);
/* Masked backward (models/models.py:57-61) from the forward's out and arg_pos: d_pre = g_out (1 - out^2) at the saved position t*,
 * g_conv_w[o][c][k] += d_pre scale X[t* + k][c], dX[t* + k][c] += d_pre scale conv_w[o][c][k], g_emb[chars[j]][c] += bit dX[j][c] (row
 * padding_idx zero; < 0: none), g_conv_b[o] += d_pre.  No floating-point atomics: every workgroup owns a fixed run of words and private
 * accumulators with one writer per cell (LDS up to 144 KiB, else its slab of the workspace), the workgroups are added in index order:
 * bitwise identical from run to run.  S == 0 writes zeros.  Two launches (and one memset when the accumulators do not fit in LDS). */
int recon_char_masked_bwd(const void* chars, int32_t index_bytes, int64_t ld_chars, const float* emb, const float* conv_w, const int32_t* bits,
                          float scale, const float* g_out, const float* out, const uint8_t* arg_pos, int64_t S, int32_t W, int32_t span,
                          int32_t cfs, int32_t V, int32_t C, int32_t Fo, int32_t padding_idx, float* g_emb, float* g_conv_w, float* g_conv_b,
                          void* workspace, size_t workspace_bytes, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * E8  The entity-context line LSTM (csrc/ctx_lstm.hip): models/models.py:56-70, one layer, two directions, batch_first, over S
 *     independent sequences of exactly T steps (no length masking: padding positions are steps like any other), h0 = c0 = 0, nn.LSTM's
 *     definition (gate order i, f, g, o; both biases added; the reverse direction walks t = T - 1 .. 0).  Only the final states are kept:
 *         out[s] = (h_fwd after t = T - 1 | h_rev after t = 0),   out [S][2 H].
 *     The input row of step t is given in two parts and never written: word_table[words[s][t]] (Dw floats; words [S][T] int32 or int64,
 *     index_bytes = 4 or 8, row stride ld_words in elements, ids outside [0, Vw) clamped into the table; Dw = 0: no such part, words and
 *     word_table may be NULL) and feat[(s T + t) ld_feat .. + Fc] (read in place, ld_feat >= Fc).  I = Dw + Fc.  w_ih [4H][I], w_hh [4H][H],
 *     b_ih, b_hh [4H] per direction (the *_rev arguments: the reverse direction's), fp32 and contiguous.  Everything is fp32 on
 *     v_mfma_f32_16x16x4_f32 (an fp32 fma chain, no reduced-precision operand).  Status codes and the 16-byte alignment of workspace and
 *     saved are those of the E7 entries.
 * ------------------------------------------------------------------------------------------*/
/* Shapes the kernels take (models/models.py:56-70): S, T, Fc >= 1, Dw >= 0, 1 <= H <= 64 (four waves of 16 hidden units), Dw + Fc <= 256,
 * T <= 2^20, and the weights of one direction (4 H (I + H) floats in the MFMA's operand layout) plus the tiles of 16 sequences within
 * 144 KiB of LDS; at most 192 16 x 16 tiles in (4 H) x (I + H + 1).  The caller runs the stock ops for anything else. */
int recon_ctx_lstm_supported(int64_t S, int32_t T, int32_t Dw, int32_t Fc, int32_t H);
/* Bytes of the workspace (models/models.py:56-70) of the forward (backward = 0: both directions' weights as the B operand, and the
 * bias sums) or of the backward (backward = 1: one private (d_w_ih | d_w_hh | d_b) per direction and workgroup, at most 128 workgroups,
 * each owning ceil(S / 128) sequences).  16-byte aligned, any contents; 0 for a shape recon_ctx_lstm_supported refuses. */
size_t recon_ctx_lstm_workspace_bytes(int64_t S, int32_t T, int32_t Dw, int32_t Fc, int32_t H, int32_t backward);
/* Bytes of the opaque buffer the forward leaves for the backward (models/models.py:56-70): the post-activation gates and the cell
 * state, 5 H floats per direction, sequence and step.  0 for a shape recon_ctx_lstm_supported refuses. */
size_t recon_ctx_lstm_saved_bytes(int64_t S, int32_t T, int32_t Dw, int32_t Fc, int32_t H);
/* Forward (models/models.py:56-70).  A workgroup owns one direction and walks tiles of 16 sequences with the direction's weights in
 * LDS; the cell state never leaves registers.  saved = NULL (no backward follows): out is the only thing written.  S == 0: nothing is
 * launched.  Two launches (operand layout, sequences). */
int recon_ctx_lstm_fwd(const void* words, int32_t index_bytes, int64_t ld_words, const float* word_table, int32_t Vw, const float* feat,
                       int64_t ld_feat, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* w_ih_rev,
                       const float* w_hh_rev, const float* b_ih_rev, const float* b_hh_rev, int64_t S, int32_t T, int32_t Dw, int32_t Fc,
                       int32_t H, float* out, void* saved, void* workspace, size_t workspace_bytes, recon_stream_t stream);
/* Backward (models/models.py:56-70) from the forward's saved buffer, which it CONSUMES (the gate gradients and h replace the gates and
 * c: one backward per forward).  g_out [S][2 H] contiguous.  d_feat [S][T][Fc] and d_word_vec [S][T][Dw] (the gradient of the gathered
 * rows, for the embedding's own backward) are contiguous; either may be NULL and is then not written.  g_b_ih and g_b_hh receive the same
 * sums.  No floating-point atomics: a pass per direction walks the steps backwards tile by tile of 16 sequences (the reverse direction's
 * launch adds its d_x to the forward direction's); then workgroup g adds
 * d_a^T (x | h | 1) over its own run of ceil(S / 128) sequences and the workgroups are added in index order: bitwise identical from
 * run to run.  S == 0 writes zeros to the eight parameter gradients and launches no kernel.  Four launches. */
int recon_ctx_lstm_bwd(const void* words, int32_t index_bytes, int64_t ld_words, const float* word_table, int32_t Vw, const float* feat,
                       int64_t ld_feat, const float* w_ih, const float* w_hh, const float* w_ih_rev, const float* w_hh_rev, const float* g_out,
                       void* saved, int64_t S, int32_t T, int32_t Dw, int32_t Fc, int32_t H, float* d_feat, float* d_word_vec, float* g_w_ih,
                       float* g_w_hh, float* g_b_ih, float* g_b_hh, float* g_w_ih_rev, float* g_w_hh_rev, float* g_b_ih_rev, float* g_b_hh_rev,
                       void* workspace, size_t workspace_bytes, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * E9  The sentence encoder's pair LSTM (csrc/sent_lstm.hip): models/models.py:160-184, one layer, two directions, batch_first, over
 *     S = B C independent sequences of exactly T steps (sequence s = b C + c is sentence b seen from entity pair c; no length masking),
 *     h0 = c0 = 0, nn.LSTM's definition as in E8.  Only the final states are kept:
 *         out[s] = (h_fwd after t = T - 1 | h_rev after t = 0),   out [B C][2 H].
 *     The input row of step t is never written: word_table[sentence[b][t]] (Dw floats; sentence [B][T], row stride ld_sentence in
 *     elements) times the dropout factors of (s, t), followed by pos_table[markers[s][t]] (P floats; markers [B C][T], row stride
 *     ld_markers).  Both id arrays are int32 or int64 (index_bytes = 4 or 8, the same for both); ids outside their table are clamped into
 *     it.  keep_bits: NULL (no dropout) or int32 [B C][T][ceil(Dw / 32)], contiguous: factor (s, t, c) = keep_scale if bit c % 32 of word
 *     c / 32 is set, else 0.  I = Dw + P.  w_ih [4H][I], w_hh [4H][H], b_ih, b_hh [4H] per direction, fp32 and contiguous.  word_table is
 *     a constant: no gradient of it is formed.  Everything is fp32 on v_mfma_f32_16x16x4_f32.  Status codes and the 16-byte alignment of
 *     workspace and saved are those of the E7 entries.
 * ------------------------------------------------------------------------------------------*/
/* Shapes the kernels take (models/models.py:160-184): B, C, T, Dw, P >= 1, 1 <= H <= 256 (eight waves of up to two 16-unit blocks),
 * Dw + P <= 128, T <= 2^20, B C T 5 H <= 2^40.  pos_table may have up to 16 rows (the fwd / bwd entries return RECON_ERR_UNSUPPORTED above,
 * workspace_bytes 0).  The caller runs the stock ops for anything else. */
int recon_sent_lstm_supported(int64_t B, int32_t C, int32_t T, int32_t Dw, int32_t P, int32_t H);
/* Bytes of the workspace (models/models.py:160-184) of the forward (backward = 0: both directions' (W_ih | W_hh)^T in the order the
 * recurrence reads its B fragments, k padded to a multiple of 16, and the bias sums) or of the backward (backward = 1: W_hh in fragment
 * order; one private (d_w_ih | d_w_hh | d_b | class sums) of 4 H (I + H + 1 + Vp) floats per direction and row group, the groups being
 * G = ceil(S / per) runs of per = ceil(S / 32) sequences; the reduced class sums).  16-byte aligned, any contents; 0 for a shape
 * recon_sent_lstm_supported refuses. */
size_t recon_sent_lstm_workspace_bytes(int64_t B, int32_t C, int32_t T, int32_t Dw, int32_t P, int32_t H, int32_t Vp, int32_t backward);
/* Bytes of the opaque buffer the forward leaves for the backward (models/models.py:160-184): the post-activation gates and the cell
 * state, 5 H floats per direction, sequence and step.  0 for a shape recon_sent_lstm_supported refuses. */
size_t recon_sent_lstm_saved_bytes(int64_t B, int32_t C, int32_t T, int32_t Dw, int32_t P, int32_t H);
/* Forward (models/models.py:160-184).  A workgroup owns one direction and one tile of sequences (16; 32 when S > 2048) for all T steps;
 * the weights come from global memory / L2 straight into registers, h goes through LDS, the cell state never leaves registers.  No
 * workgroup waits for another.  saved = NULL (no backward follows): out is the only thing written.  B C == 0: nothing is launched.
 * Two launches (operand layout, sequences). */
int recon_sent_lstm_fwd(const void* sentence, const void* markers, int32_t index_bytes, int64_t ld_sentence, int64_t ld_markers,
                        const float* word_table, int32_t Vw, const float* pos_table, int32_t Vp, const int32_t* keep_bits, float keep_scale,
                        const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* w_ih_rev, const float* w_hh_rev,
                        const float* b_ih_rev, const float* b_hh_rev, int64_t B, int32_t C, int32_t T, int32_t Dw, int32_t P, int32_t H,
                        float* out, void* saved, void* workspace, size_t workspace_bytes, recon_stream_t stream);
/* Backward (models/models.py:160-184) from the forward's saved buffer, which it CONSUMES (the gate gradients and h replace the gates and
 * c: one backward per forward).  g_out [B C][2 H] contiguous.  g_pos_table [Vp][P] receives the gradient of pos_table, row
 * pos_padding_idx zero (< 0: none), formed as (sum of d_a over the rows of each marker value) . W_ih[:, Dw:]; no d_x is written.  g_b_ih
 * and g_b_hh receive the same sums.  No floating-point atomics: a pass walks the steps backwards tile by tile; then workgroup
 * (g, block of 128 gate rows, direction) adds d_a^T (x | h | 1 | onehot(marker)) over row group g and the groups are added in index
 * order: bitwise identical from run to run.  B C == 0 writes zeros to the nine gradients and launches no kernel.  Five launches. */
int recon_sent_lstm_bwd(const void* sentence, const void* markers, int32_t index_bytes, int64_t ld_sentence, int64_t ld_markers,
                        const float* word_table, int32_t Vw, const float* pos_table, int32_t Vp, const int32_t* keep_bits, float keep_scale,
                        const float* w_ih, const float* w_hh, const float* w_ih_rev, const float* w_hh_rev, const float* g_out, void* saved,
                        int64_t B, int32_t C, int32_t T, int32_t Dw, int32_t P, int32_t H, int32_t pos_padding_idx, float* g_pos_table,
                        float* g_w_ih, float* g_w_hh, float* g_b_ih, float* g_b_hh, float* g_w_ih_rev, float* g_w_hh_rev, float* g_b_ih_rev,
                        float* g_b_hh_rev, void* workspace, size_t workspace_bytes, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * E10 The pair states' transition projections (csrc/pair_trans.hip): the L per-hop projections of the pair states in front of the
 *     propagation, T_l = act(x W_l^T + b_l) for l < L  (GPGNN models/models.py:185-192 tied, :240-249 untied; RECON_EAC :395-402 and
 *     :450-459; RECON_EAC_KGGAT :605-612 and :660-669; RECON :843-850 and :898-907).  x [M][K] with row stride ld_x (elements), W_l
 *     [N1][K], b_l [N1], out[l] and g_out[l] [M][N1], all fp32; everything but x contiguous.  w, b, out, g_out, g_w, g_b are HOST arrays of L
 *     device pointers (like recon_prop_args.adj).  act is RECON_ACT_*; act' is taken from the OUTPUT (relu T > 0, tanh 1 - T^2, linear 1)
 *     and d_pre_l = g_out[l] act'(out[l]) is formed while an operand is staged, never written.  Everything is fp32 on
 *     v_mfma_f32_16x16x4_f32, without atomics, every sum in an order the shape alone decides: bitwise identical from run to run.  Status
 *     codes and the 16-byte alignment of workspace are those of the E8 / E9 entries.
 * ------------------------------------------------------------------------------------------*/
/* Shapes the kernels take (models/models.py:185-192, :240-249): 0 <= M <= 2^24, K a multiple of 4 in 4..1024, 1 <= N1 <= 1024,
 * 1 <= L <= 8.  The fwd / bwd entries also need 16-byte aligned x and W_l and ld_x % 4 == 0.  Everything else answers
 * RECON_ERR_UNSUPPORTED and writes nothing; the caller then runs the stock ops. */
int recon_pair_transitions_supported(int64_t M, int32_t K, int32_t N1, int32_t L);
/* Bytes of the workspace (models/models.py:185-192, :240-249).  Forward (backward = 0): none.  Backward (backward = 1): G slabs of
 * L N1 (K + 1) floats, one per row group, where G = min(8, ceil(M / 32)) and a group is per = ceil(M / G) consecutive rows: a function of
 * M alone.  16-byte aligned, any contents; 0 for a shape recon_pair_transitions_supported refuses and for M == 0. */
size_t recon_pair_transitions_workspace_bytes(int64_t M, int32_t K, int32_t N1, int32_t L, int32_t backward);
/* Forward (models/models.py:185-192, :240-249; the other models' lines above): [M][K] x [K][L N1] in 64 x 64 tiles, the bias (b NULL or
 * b[l] NULL: none) and the activation in the epilogue, stored into out[l].  A column tile may straddle a layer boundary.  M == 0: nothing
 * is launched.  One launch. */
int recon_pair_transitions_fwd(const float* x, int64_t ld_x, const float* const* w, const float* const* b, int64_t M, int32_t K, int32_t N1,
                               int32_t L, int32_t act, float* const* out, recon_stream_t stream);
/* Backward (models/models.py:185-192, :240-249) from the forward's outputs, which it leaves as they are (any number of backwards per
 * forward, the same bits each time).  g_out[l] NULL: that output received no gradient; the layer adds nothing to g_x and its wanted
 * parameter gradients receive zeros.  g_x [M][K] contiguous or NULL (not wanted: its launch is skipped) = sum_l d_pre_l W_l, reduced in
 * the order l ascending, n ascending.  g_w[l] [N1][K] and g_b[l] [N1] (g_w, g_b or single entries NULL: not wanted; no entry wanted: both
 * launches are skipped) = d_pre_l^T (x | 1): workgroup (column tile, layer and row tile, g) writes its part of slab g of the workspace
 * over row group g, then the slabs are added in group order.  M == 0 writes zeros to every wanted gradient and launches no kernel.
 * Three launches: one for g_x, two for the parameters. */
int recon_pair_transitions_bwd(const float* x, int64_t ld_x, const float* const* w, const float* const* out, const float* const* g_out,
                               int64_t M, int32_t K, int32_t N1, int32_t L, int32_t act, float* g_x, float* const* g_w, float* const* g_b,
                               void* workspace, size_t workspace_bytes, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * E11 The relation classifier over its feature blocks (csrc/rel_head.hip): the head between the propagation and the logits,
 *     logits = cat(block_0 .. block_{n-1}, S) W^T + b  (GPGNN and RECON_EAC models/models.py:213, :234, :275: one block; RECON_EAC_KGGAT
 *     :693-697: the propagation features and the KB-GAT columns; RECON :954-966: those two and the scattered translation scores), without
 *     the concatenated operand.  blocks, ld and widths are HOST arrays of n_blocks entries: device pointer, row stride (elements) and
 *     width K_i >= 1 of block i, [M][K_i]; they travel by value in the kernel arguments.  The scattered block S [M][K_s] is given by
 *     scattered [Mnz][K_s] (row stride ld_s) and positions [Mnz] (int64, STRICTLY INCREASING, inside [0, M)): row positions[i] of S is
 *     scattered[i], every other row is zero (the zeros + index_put of :954-958).  K_s == 0: no such block; Mnz == 0: an all-zero block,
 *     scattered and positions are not read.  A position outside [0, M) is never used as an address: the kernels ignore such a row.  W
 *     [N][Kt] with Kt = sum K_i + K_s, b [N] or NULL, out and g_out [M][N], all fp32; W, b, out, g_out and the gradients contiguous.  No
 *     width, stride or base needs more than 4-byte alignment: a block (or a block's weight columns) whose base, stride and width are
 *     4-aligned is read as float4, any other element by element (per block in the backward; in the forward one such block puts the
 *     operand's loads of the whole call on the element form).  Everything is fp32 on v_mfma_f32_16x16x4_f32, without atomics, every
 *     sum in an order the shapes and the positions decide: bitwise identical from run to run.  Status codes and the 16-byte alignment of
 *     workspace are those of the E8 - E10 entries.
 * ------------------------------------------------------------------------------------------*/
/* Shapes the kernels take (models/models.py:213, :234, :275, :693-697, :954-966): 0 <= M <= 2^24, 1 <= n_blocks <= 4 dense blocks (plus
 * the scattered one), 1 <= Kt <= 2048 for the weight's row length, 1 <= N <= 1024.  Everything else answers RECON_ERR_UNSUPPORTED and
 * writes nothing; the caller then runs the stock ops. */
int recon_relation_logits_supported(int64_t M, int32_t n_blocks, int32_t Kt, int32_t N);
/* Bytes of the workspace (models/models.py:213, :234, :275, :693-697, :954-966).  Forward (backward = 0): none.  Backward
 * (backward = 1): G slabs of N (Kt + 1) floats, one per row group, where G = min(8, ceil(M / 32)) and a group is per = ceil(M / G)
 * consecutive rows: a function of M alone.  16-byte aligned, any contents; 0 for a shape recon_relation_logits_supported refuses and
 * for M == 0. */
size_t recon_relation_logits_workspace_bytes(int64_t M, int32_t n_blocks, int32_t Kt, int32_t N, int32_t backward);
/* Forward (models/models.py:213, :234, :275, :693-697, :954-966): [M][Kt] x [Kt][N] in 64 x 64 tiles with the bias (NULL: none) in the
 * epilogue.  The reduction walks the blocks in order, 32 columns per step, a step inside ONE block (a block's last step is filled with
 * zeros); whether a staged row is present in the scattered block is one binary search over positions per thread.  M == 0: nothing is
 * launched.  One launch. */
int recon_relation_logits_fwd(const float* const* blocks, const int64_t* ld, const int32_t* widths, int32_t n_blocks, const float* scattered,
                              int64_t ld_s, int32_t K_s, const int64_t* positions, int64_t Mnz, const float* weight, const float* bias, int64_t M,
                              int32_t N, float* out, recon_stream_t stream);
/* Backward (models/models.py:213, :234, :275, :693-697, :954-966); it destroys nothing (any number of backwards per forward, the same bits
 * each time).  g_blocks: HOST array of n_blocks device pointers, g_blocks[i] [M][K_i] contiguous = g_out W[:, cols_i], or NULL (g_blocks
 * itself or an entry: not wanted, no work is done for it); g_scattered [Mnz][K_s] contiguous or NULL: row i = g_out[positions[i]]
 * W[:, cols_s] (zeros for a position outside [0, M)); one launch over the column tiles of the wanted blocks, skipped when there is none.
 * g_w [N][Kt] and g_b [N] (NULL: not wanted; both NULL: both launches are skipped) = g_out^T (cat | 1): workgroup (column tile, row tile,
 * z) writes its part of slab z of the workspace over row group z — for the scattered block over the present rows of the group alone —
 * then the slabs are added in group order.  M == 0 writes zeros to every wanted gradient and launches no kernel.  At most three launches. */
int recon_relation_logits_bwd(const float* const* blocks, const int64_t* ld, const int32_t* widths, int32_t n_blocks, const float* scattered,
                              int64_t ld_s, int32_t K_s, const int64_t* positions, int64_t Mnz, const float* weight, const float* g_out, int64_t M,
                              int32_t N, float* const* g_blocks, float* g_scattered, float* g_w, float* g_b, void* workspace,
                              size_t workspace_bytes, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * E12 The entity-level tail of the entity-context encoder (csrc/line_pool.hip): conv1d_entity over the line states, the line mask and
 *     the max over the lines (models/models.py:73-81) as one op:
 *     out[u][e] = max over unmasked p of  bias[e] + sum_{j < k} sum_c weight[e][c][j] states[u][p + j][c],   P = Ln - k + 1 positions.
 *     states: U Ln rows of C floats at ONE row stride ld >= C (elements), entity u's line l at row u Ln + l; weight [E][C][k]
 *     (nn.Conv1d's layout), bias [E], out and g_out [U][E], all fp32 and contiguous but for ld; mask [U][P] bytes, nonzero = padding
 *     position, any pattern.  An exact tie takes the lowest position; an entity without an unmasked position gives -inf and no gradient;
 *     a NaN at an unmasked position gives NaN.  positions [U][E] bytes: the winning position, 255 for none.  Everything is fp32 on the
 *     VALU, without atomics, every sum in an order the shapes alone decide: bitwise identical from run to run.  Neither the [U][E][P]
 *     convolution output nor its masked copy exists.  Status codes and the 16-byte alignment of workspace are those of the E8 - E11
 *     entries; nothing is allocated inside the library.
 * ------------------------------------------------------------------------------------------*/
/* Shapes the kernels take (models/models.py:73-81): 0 <= U <= 2^30, 1 <= k <= Ln, P = Ln - k + 1 <= 255 (the position byte), C k <= 1024,
 * 1 <= E <= 64.  Everything else answers RECON_ERR_UNSUPPORTED and writes nothing; the caller then runs the stock ops. */
int recon_line_pool_supported(int64_t U, int32_t Ln, int32_t C, int32_t E, int32_t k);
/* Bytes of the backward's workspace (models/models.py:73-81): G slabs of E (C k + 1) floats, one per entity group, where
 * per = ceil(U / min(256, U)) consecutive entities make a group and G = ceil(U / per): a function of U alone.  16-byte aligned, any
 * contents; 0 for a shape recon_line_pool_supported refuses and for U == 0.  The forward needs none. */
size_t recon_line_pool_workspace_bytes(int64_t U, int32_t Ln, int32_t C, int32_t E, int32_t k);
/* Forward (models/models.py:73-81): one workgroup per entity stages the weight and the entity's line states in LDS (in chunks where they
 * do not fit), forms every (position, channel) sum as one fma chain over j then c, adds the bias and keeps the first maximum among the
 * unmasked positions.  positions may be NULL (no backward will follow): then only out is written.  U == 0: nothing is launched.  One
 * launch. */
int recon_line_pool_fwd(const float* states, int64_t ld, const float* weight, const float* bias, const void* mask, int64_t U, int32_t Ln,
                        int32_t C, int32_t E, int32_t k, float* out, void* positions, recon_stream_t stream);
/* Backward (models/models.py:73-81); it destroys nothing (any number of backwards per forward, the same bits each time).
 * g_states [U][Ln][C] contiguous or NULL: d_states[u][l][c] = sum over e ascending of [0 <= l - pos[u][e] < k] g_out[u][e]
 * weight[e][c][l - pos[u][e]]; every cell is written once, zeros included.  g_w [E][C][k] and g_b [E] (NULL: not wanted; both NULL: the
 * slab work and the second launch are skipped): d_weight[e][c][j] = sum_u g_out[u][e] states[u][pos[u][e] + j][c], d_bias[e] = sum_u
 * [pos[u][e] != 255] g_out[u][e], each entity group summed upwards into its slab of the workspace, the slabs added in group order.
 * U == 0 writes zeros to g_w and g_b and launches no kernel.  At most two launches. */
int recon_line_pool_bwd(const float* states, int64_t ld, const float* weight, const float* g_out, const void* positions, int64_t U,
                        int32_t Ln, int32_t C, int32_t E, int32_t k, float* g_states, float* g_w, float* g_b, void* workspace,
                        size_t workspace_bytes, recon_stream_t stream);
/* The ragged form of E12 (models/models.py:73-81 over the present lines alone): states is a flat list of L rows of C floats at one row
 * stride ld >= C, and entity u owns the rows line_ptr[u] .. line_ptr[u + 1] (int32 [U + 1], ascending, line_ptr[0] = 0, line_ptr[U] = L;
 * n_max = the longest entity's rows).  Every row is a present line, so no mask is read:
 *     out[u][e] = max over p < n_u - k + 1 of  bias[e] + sum_{j < k} sum_c weight[e][c][j] states[line_ptr[u] + p + j][c]
 * which is what the padded form gives for the same entity with the positions p >= n_u - k + 1 masked, bit for bit (a cell's sum is one
 * fma chain whose order does not depend on the chunk sizes).  An entity with n_u < k rows (n_u = 0 included) gives -inf, position byte
 * 255 and no gradient.  Shapes: 0 <= U <= 2^30, 0 <= n_max <= L <= U n_max, L < 2^31, n_max - k + 1 <= 255, C k <= 1024, 1 <= E <= 64,
 * k >= 1; everything else answers RECON_ERR_UNSUPPORTED (negative sizes RECON_ERR_INVALID) before any launch. */
int recon_line_pool_ragged_supported(int64_t U, int64_t L, int32_t n_max, int32_t C, int32_t E, int32_t k);
/* Bytes of the ragged backward's workspace (models/models.py:73-81): the G slabs of recon_line_pool_workspace_bytes, G a function of U
 * alone; 0 for a refused shape and for U == 0. */
size_t recon_line_pool_ragged_workspace_bytes(int64_t U, int64_t L, int32_t n_max, int32_t C, int32_t E, int32_t k);
/* Ragged forward (models/models.py:73-81): recon_line_pool_fwd's kernel instantiated with the row base and the position count taken from
 * line_ptr; out [U][E], positions [U][E] bytes or NULL.  states may be NULL when L == 0.  One launch. */
int recon_line_pool_ragged_fwd(const float* states, int64_t ld, const float* weight, const float* bias, const int32_t* line_ptr, int64_t U,
                               int64_t L, int32_t n_max, int32_t C, int32_t E, int32_t k, float* out, void* positions, recon_stream_t stream);
/* Ragged backward (models/models.py:73-81): recon_line_pool_bwd's kernels over the same entity groups.  g_states [L][C] contiguous or
 * NULL, every cell written once; g_w, g_b, the workspace and the launches as there; no atomics, bitwise reproducible, any number of
 * backwards per forward. */
int recon_line_pool_ragged_bwd(const float* states, int64_t ld, const float* weight, const float* g_out, const void* positions,
                               const int32_t* line_ptr, int64_t U, int64_t L, int32_t n_max, int32_t C, int32_t E, int32_t k, float* g_states,
                               float* g_w, float* g_b, void* workspace, size_t workspace_bytes, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * E13 The stage-B objective between the logits and the optimiser (csrc/objective.hip): CrossEntropyLoss(ignore_index) over [M][n_out],
 *     torch.max's indices, the softmax probability of the prediction and the counters of evaluate_instance_based (train.py:232,
 *     :309-324, test.py:274-291, utils/evaluation_utils.py:17-59) without the [M][n_out] log-softmax and without a host read:
 *     lse[m] = log sum_c exp(x[m][c] - max_m) (the row's log-sum-exp LESS its maximum: with the maximum added in fp32 the backward's
 *     softmax would carry the maximum's rounding; the backward takes the maximum, which is exact, from the row again),
 *     term[m] = lse[m] - (x[m][labels[m]] - max_m), loss = (sum of the kept rows' terms, row order, fp64, rounded once) / kept, where a
 *     row is kept when labels[m] != ignore_index; predicted[m] = the lowest index of the row's
 *     maximum, a NaN counting as the maximum (the lowest NaN); confidence[m] = 1 / sum_c exp(x[m][c] - max_m); counts = {kept, n_pred,
 *     n_gold, n_ok} over the kept rows: predicted != empty_label, labels != empty_label, predicted == labels != empty_label;
 *     prec = n_ok / n_pred and rec = n_ok / n_gold (0 where the denominator is 0), f1 = 2.0 prec rec / (prec + rec) in that order in
 *     fp64 (0 where prec + rec == 0).  kept == 0: loss NaN (0 / 0).  A kept row whose label lies outside [0, n_out) has the term NaN, a
 *     zero gradient row and counts as gold; its label is never used as an address.  +inf, -inf and NaN in a row go through the plain
 *     arithmetic above, which is log_softmax's.  logits: M rows of n_out floats at ONE row stride ld >= n_out (elements); labels [M]
 *     int64; predicted [M] int64; confidence, lse [M] fp32; loss [1] fp32; counts [4] int64; f1 [1] fp64; g_logits [M][n_out] contiguous.
 *     No atomics, every sum in an order M and n_out decide: bitwise identical from run to run.  Status codes and the 16-byte alignment of
 *     workspace are those of the E8 - E12 entries; nothing is allocated inside the library.
 * ------------------------------------------------------------------------------------------*/
/* Shapes the kernels take (train.py:232, train.py:309-324, test.py:274-291, utils/evaluation_utils.py:17-59): 0 <= M <= 2^30,
 * 1 <= n_out <= 8192 (a row up to 512 wide is held in registers, a wider one is walked twice).  Everything else answers
 * RECON_ERR_UNSUPPORTED and writes nothing; the caller then runs the stock ops. */
int recon_relation_objective_supported(int64_t M, int32_t n_out);
/* Bytes of the forward's workspace (train.py:232, train.py:309-324, test.py:274-291, utils/evaluation_utils.py:17-59): the M row terms,
 * fp32.  16-byte aligned, any contents; 0 for a shape recon_relation_objective_supported refuses and for M == 0.  Not needed with
 * labels == NULL.  The backward needs none. */
size_t recon_relation_objective_workspace_bytes(int64_t M, int32_t n_out);
/* Forward (train.py:232, train.py:309-324, test.py:274-291, utils/evaluation_utils.py:17-59).  First launch: a wavefront per row writes
 * predicted, confidence, the row's term into the workspace and, when lse != NULL (a backward will follow), the row's lse as defined above.
 * Second launch: one workgroup adds the kept rows' terms in a fixed order, counts, and writes loss, counts and f1; with acc_counts [4]
 * int64, acc_f1_sum [1] fp64 and acc_batches [1] int64 (all three or none) it also adds counts, f1 and 1 to them, so that an epoch's
 * sums stay on the device: acc_f1_sum holds the bits of the reference's `f1 += add_f1` over the same batches in the same order.
 * labels == NULL is the test-time form: predicted and confidence alone, one launch; loss, lse, counts, f1 and the accumulator must then
 * be NULL.  M == 0: nothing is launched and nothing is written. */
int recon_relation_objective_fwd(const float* logits, int64_t ld, const int64_t* labels, int64_t M, int32_t n_out, int64_t ignore_index,
                                 int64_t empty_label, float* loss, int64_t* predicted, float* confidence, float* lse, int64_t* counts,
                                 double* f1, int64_t* acc_counts, double* acc_f1_sum, int64_t* acc_batches, void* workspace,
                                 size_t workspace_bytes, recon_stream_t stream);
/* Backward (train.py:232, train.py:309-324, test.py:274-291, utils/evaluation_utils.py:17-59); it destroys nothing (any number of
 * backwards per forward, the same bits each time).  g_logits[m][c] = g_loss[0] (exp((x[m][c] - max_m) - lse[m]) - [c == labels[m]]) / counts[0] for
 * a kept row with a label inside [0, n_out); a zero row for an ignored row and for a label outside; all zeros when counts[0] == 0.
 * g_loss [1] fp32 (the incoming gradient of loss) and counts (the forward's) are read on the device: the host never learns kept.  Every
 * cell is written exactly once.  M == 0: nothing is launched.  One launch. */
int recon_relation_objective_bwd(const float* logits, int64_t ld, const int64_t* labels, const float* lse, const float* g_loss,
                                 const int64_t* counts, int64_t M, int32_t n_out, int64_t ignore_index, float* g_logits,
                                 recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * E2  KG training of the ConvKB scorer (csrc/kg_train.hip): stage B of KB-GAT, train_conv (GAT/main.py:707-860), over frozen tables.
 *     Indices: int32 or int64 [rows][3] = (head, relation, tail), index_bytes = 4 or 8.
 * ------------------------------------------------------------------------------------------*/
/* Filtered corruption: the negative half of Corpus.get_iteration_batch (GAT/create_batch.py:103-260) and get_iteration_triples_batch
 * (:262-351) for B positives and ratio r >= 0.  Writes indices int64 [B (2 r + 1)][3] and out_values [B (2 r + 1)]: rows 0..B are the
 * positives; row B + c starts as a copy of positive c mod B (np.tile, :126-129) and replaces the head for c in [0, B (r/2)) (:131-141), the
 * tail for c in [B (r/2), 2 B (r/2)) (:143-155), the relation for c in [B r, 2 B r) (:157-174); for odd r the rows c in [2 B (r/2), B r)
 * stay copies.  A replaced row has value -1.  Entity draws are uniform over [0, n_ent), redrawn while (h, r, t) is known; a row still known
 * after 65 536 draws stays a copy with the positive's value and adds 1 to *capped (device, never reset by the library).  Relation draws:
 * at most n_rel membership checks, then the row keeps the positive's relation and value (:163-174).  Known: keys = sorted unique int64
 * (r n_ent + h) n_ent + t of train + valid + test (valid_triples_dict).  Draw k of row c is a counter-based function of (seed, c, k):
 * the output is bit-reproducible for a seed.  Positive ids are not range-checked (the caller does it); nothing is read outside keys. */
int recon_kg_corrupt(const void* positives, int32_t index_bytes, const float* values, int64_t B, int32_t ratio, const int64_t* keys,
                     int64_t n_keys, int64_t n_ent, int64_t n_rel, uint64_t seed, int64_t* indices, float* out_values,
                     unsigned long long* capped, recon_stream_t stream);
/* ConvKB training forward (SpKBGATConvOnly.forward, GAT/models.py:291-296 -> ConvKB.forward, GAT/layers.py:41-46) on M triples, the
 * tables E [n_ent][D] and Rel [n_rel][D] read in place (no torch.cat): z = [E[h] | Rel[r] | E[t]] W1^T + b1 (W1 [D][3 D]),
 * scores = leaky(z) . w2 + b2, leaky(x) = max(x, slope x), 0 <= slope <= 1.  1 <= D <= 512 (RECON_ERR_UNSUPPORTED above).  z [M][D]
 * (optional, NULL: not written) is what recon_convkb_train_bwd needs.  fp32 fma chains, no split precision.  A row with an id outside
 * its table scores NaN; nothing is read outside a table.
 * With values [M] (+1 / -1, optional) and ratio >= 1 it also computes main.py:833-840's loss: y = (v + 1) / 2, w = y + (1 - y) / (2 ratio),
 * loss[0] = mean_m w_m ((1 - y_m) s_m + mx + log(exp(-mx) + exp(-s_m - mx))), mx = max(-s_m, 0) (binary_cross_entropy_with_logits,
 * weight = w), loss_terms [M] (optional) the weighted terms, g_scores [M] = dloss/ds = w (sigmoid(s) - y) / M.  The mean is a fixed-order
 * sum.  workspace: recon_convkb_train_fwd_workspace_floats(M, D) floats, zero-filled before its first use; only needed with values.
 * One launch. */
size_t recon_convkb_train_fwd_workspace_floats(int64_t M, int32_t D);
int recon_convkb_train_fwd(const void* triples, int32_t index_bytes, int64_t M, const float* E, const float* Rel, int64_t n_ent, int64_t n_rel,
                           int32_t D, const float* W1, const float* b1, const float* w2, const float* b2, float slope, float* z, float* scores,
                           const float* values, int32_t ratio, float* loss_terms, float* g_scores, float* loss, float* workspace,
                           size_t workspace_floats, recon_stream_t stream);
/* ConvKB training backward (loss.backward() of main.py:842 through fc2, nl1 and fc1; the tables are frozen, :741-742): g = g_scores
 * (* g_scale[0] when g_scale is given), delta = (g w2) * (z > 0 ? 1 : slope), dW1 [D][3 D] = delta^T X with X gathered again, db1 = sum_m
 * delta, dw2 [D] = sum_m g leaky(z), db2 [1] = sum_m g.  Every sum has one fixed order: the gradients are bitwise identical from run to run.
 * workspace: recon_convkb_train_bwd_workspace_floats(M, D) floats, zero-filled before its first use.  One launch.
 * Both workspaces begin with the same 256 arrival counters, which every call leaves at zero: one zero-filled buffer of the largest size
 * asked for serves every shape, forward and backward alike (not two calls in flight on different streams at once). */
size_t recon_convkb_train_bwd_workspace_floats(int64_t M, int32_t D);
int recon_convkb_train_bwd(const void* triples, int32_t index_bytes, int64_t M, const float* E, const float* Rel, int64_t n_ent, int64_t n_rel,
                           int32_t D, const float* w2, float slope, const float* z, const float* g_scores, const float* g_scale, float* dW1,
                           float* db1, float* dw2, float* db2, float* workspace, size_t workspace_floats, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * E6  Parameter updates (csrc/optim.hip): the optimizer steps of the three training programs as multi-tensor launches.
 *     A step is a list of n_segments segments: host arrays of DEVICE pointers (parameter, gradient, state), one entry per segment, and a
 *     host array numel of element counts.  Everything is fp32 and contiguous; a pointer needs 4-byte alignment only (segments whose
 *     pointers are all 16-byte aligned move 16 bytes per lane, the others 4); the buffers of a segment must not overlap.  The segment
 *     descriptors travel in the kernel arguments: the host arrays are read during the call and may be reused as soon as it returns, and
 *     no device table exists.  One launch takes recon_optim_max_segments() segments (and a segment above 2^30 elements counts as one per
 *     2^30); longer lists are spread over several launches.  Each workgroup owns one run of recon_optim_chunk_elems() elements.
 *     Every entry point: RECON_ERR_INVALID for n_segments < 0, a negative count, or a NULL array or NULL segment pointer where there are
 *     elements; RECON_OK with nothing launched and nothing written for n_segments == 0 or all counts 0.
 * ------------------------------------------------------------------------------------------*/
int32_t recon_optim_max_segments(void);
int32_t recon_optim_chunk_elems(void);
/* Bytes of recon_optim_grad_sumsq's workspace for a step of n_segments gradients with total_elems elements in all: 16 bytes of results
 * and one 8-byte word per workgroup.  16-byte aligned, ZERO-FILLED before its first use (the arrival counter; every call leaves it at 0). */
size_t recon_optim_workspace_bytes(int64_t total_elems, int32_t n_segments);
/* clip_grad_norm(parameters, max_norm) without the scaling pass (train.py:314-315; torch.nn.utils.clip_grad_norm_, norm_type 2):
 * workspace float [0] = total_norm = sqrt(sum over every element of every gradient of g^2), float [1] = the scale
 * min(1, max_norm / (total_norm + 1e-6)) that recon_optim_sgd / recon_optim_adam take as clip_scale.  The gradients are not modified.
 * Squares and sums in fp64; every workgroup leaves its sum in its own word, the one that arrives last adds all words in index order:
 * bitwise identical from run to run.  A non-finite gradient gives a non-finite norm and scale (error_if_nonfinite=False).  The host
 * never waits: both values stay on the device.  One launch per recon_optim_max_segments() segments. */
int recon_optim_grad_sumsq(const void* const* grads, const int64_t* numel, int32_t n_segments, float max_norm, void* workspace,
                           size_t workspace_bytes, recon_stream_t stream);
/* torch.optim.SGD(lr, weight_decay).step() (GAT/main.py:445-449; no momentum): g' = s g + weight_decay p, p <- p - lr g', with s = *clip_scale
 * (device; NULL: 1).  One launch per recon_optim_max_segments() segments. */
int recon_optim_sgd(void* const* params, const void* const* grads, const int64_t* numel, int32_t n_segments, double lr, double weight_decay,
                    const float* clip_scale, recon_stream_t stream);
/* torch.optim.Adam(lr, betas, eps, weight_decay).step() (GAT/main.py:747-751, train.py:234; L2 decay folded into the gradient, not AdamW,
 * no amsgrad): g' = s g + weight_decay p, m <- beta1 m + (1 - beta1) g', v <- beta2 v + (1 - beta2) g'^2,
 * p <- p - (lr / bias_correction1) m / (sqrt(v) / sqrt(bias_correction2) + eps), with bias_correction_i = 1 - beta_i^t for the step count t
 * AFTER this step, computed by the caller in double precision (both > 0, else RECON_ERR_INVALID), and s = *clip_scale (device; NULL: 1).
 * Evaluated in fp32 in the operation order of torch's single-tensor implementation (m by lerp: m + (1 - beta1) (g' - m)), rounding for
 * rounding.  Every segment of a call shares t.  One launch per recon_optim_max_segments() segments. */
int recon_optim_adam(void* const* params, const void* const* grads, void* const* exp_avg, void* const* exp_avg_sq, const int64_t* numel,
                     int32_t n_segments, double lr, double beta1, double beta2, double eps, double weight_decay, double bias_correction1,
                     double bias_correction2, const float* clip_scale, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * E14  The stage-B entity-context batch (csrc/ctx_batch.hip): what train.py:250-258 (again :337-344, and test.py) builds on the host for
 *      every batch — utils/context_utils.py:62-84 get_batch_unique_entities, :293-301 get_entity_location_unique_entities, :365-385
 *      get_context_indices, :444-475 get_gat_entity_embeddings / get_selected_gat_entity_embeddings — from tables built once per dataset
 *      (recon_amd/context_batch.py).  Selection, ordering and copying only: integers to the value, floats to the bit.
 *      tables: a HOST array of 11 DEVICE pointers, int32 unless said otherwise, none of them empty —
 *        0 ent_line_ptr [Ne + 2]   the table lines of entity id e are [ptr[e + 1], ptr[e + 2]); e = -1 (ALL_ZERO) is row 0
 *        1 ent_max_len  [Ne + 1]   tokens of the longest table line of id e, at e + 1 (0 without lines; -1: no entity has this id)
 *        2 line_start, 3 line_len [L]    a line's tokens are tok_flat[start .. start + len), len already cut at max_sent_len
 *        4 sf_start, 5 sf_len [S]        the same for a surface form; surface 0 is ['ALL_ZERO']
 *        6 tok_flat     token ids       7 tok_word [V] word id of a token (embedding_utils.get_idx)
 *        8 tok_chars [V][max_char_len]   char ids of its first max_char_len characters, the pad char behind its end
 *        9 gat_row [Ne + 1]   at e + 1: row of gat_emb, -1: a zero row, -2: not in gat_entity2idx (NULL without a GAT table)
 *       10 gat_emb fp32 [Ng][G]          (NULL without a GAT table)
 *      dims: a HOST array of 12 int64 — Ne, S, V, L, len(tok_flat), max_sent_len, max_num_contexts, max_char_len, conv_filter_size,
 *        the pad char id, G, Ng.  Both arrays are read during the call only.
 *      Every entry: RECON_ERR_INVALID for a NULL pointer, n_pairs < 1 or a dimension out of range, RECON_ERR_UNSUPPORTED above
 *      recon_ctx_batch_supported's limit, both before any launch.  No allocation, no global atomics, bitwise reproducible.
 * ------------------------------------------------------------------------------------------*/
/* 1 when a batch of n_ids = 2 B C entity ids runs in the kernels (train.py:250-258): n_ids even, 2 <= n_ids <= 8192 (16 bytes of LDS hash
 * table per id plus 2 KiB of bitmap and scan, of the 160 KiB of a workgroup; the reference's batch is 7200), num_entities < 2^31 - 1,
 * 1 <= num_surfaces < 2^31. */
int recon_ctx_batch_supported(int64_t n_ids, int64_t num_entities, int64_t num_surfaces);
/* get_batch_unique_entities + get_entity_location_unique_entities (train.py:250-258; utils/context_utils.py:62-84, :293-301) and the
 * presence scan of get_selected_gat_entity_embeddings (:455-475), one workgroup, one launch.  entity_indices int64 [n_pairs][2] with
 * values -1 .. Ne - 1, surface_ids int32 [n_pairs][2].  Writes unique_entities int64 [<= 2 n_pairs + 1]: -1, then the ids in order of
 * first occurrence; unique_info int32 [<= 2 n_pairs + 1][2] = (lines of the entity with its surface form, surface id of its LAST
 * occurrence; 0 for a -1 that does not occur); entities_position int64 [n_pairs][2]; with gat_mode 2 ('selected')
 * nonzero_entity_pos int64 [<= n_pairs], the pairs with a half other than -1 in row order, and pair_slot int32 [n_pairs], a pair's row
 * among them or -1 (all -1 for gat_mode 0, none, and 1, 'all'); header int32 [8] = U, T_b, P_b, Mnz, the position of the first maximum
 * of the occurrence counts, flags, L = the sum over the unique entities of min(lines, max_num_contexts) (the rows of the ragged form,
 * recon_ctx_batch_fill_ragged; the padded form does not read it), 0.  Flags: 1 an id outside [-1, Ne) or without an entity, 2 a surface id outside [0, S), 4 a pair with exactly one -1
 * half (gat_mode 2), 8 an entity whose gat_row is -2 (gat_mode 1, 2).  A flagged value is never used as an address; its outputs are
 * unspecified and the host must not launch the other two entries. */
int recon_ctx_batch_index(const void* const* tables, const int64_t* dims, const int64_t* entity_indices, const int32_t* surface_ids,
                          int64_t n_pairs, int32_t gat_mode, int64_t* unique_entities, int32_t* unique_info, int64_t* entities_position,
                          int64_t* nonzero_entity_pos, int32_t* pair_slot, int32_t* header, recon_stream_t stream);
/* get_context_indices (train.py:250-258; utils/context_utils.py:365-385 over :120-152, :256-291) for the U unique entities of
 * recon_ctx_batch_index: context_words [U][P_b][T_b] and context_chars [U][P_b][cfs - 1 + T_b (max_char_len + cfs - 1)] of
 * index_bytes = 4 or 8 (int32 / int64), context_mask bool [U][P_b] (1 from the entity's line count on).  Line 0 is the surface form,
 * lines 1.. the table's; pad word 0, pad char dims[9].  Every cell is written exactly once, as runs of 16-byte stores (element stores
 * at an unaligned array's two ends).  RECON_ERR_UNSUPPORTED for a char block of 2^31 - 4096 cells or more.  One launch. */
int recon_ctx_batch_fill(const void* const* tables, const int64_t* dims, const int64_t* unique_entities, const int32_t* unique_info, int64_t U,
                         int32_t P_b, int32_t T_b, int32_t index_bytes, void* context_words, void* context_chars, void* context_mask,
                         recon_stream_t stream);
/* get_context_indices without its padding lines (train.py:250-258; utils/context_utils.py:365-385 pads every entity to the batch's
 * richest, :285-291 get_mask marks the first n_u lines present): context_words [L][T_b] and context_chars [L][cfs - 1 + T_b
 * (max_char_len + cfs - 1)], entity u's n_u = min(lines, P_b) rows one after another in rank order, L = header[6] of
 * recon_ctx_batch_index.  Writes line_ptr int32 [U + 1], the exclusive scan of the n_u (line_ptr[U] = L), and row_entity int32 [L], the
 * owner of every row, which the fill reads to place a row; both stay valid for the caller (line_ptr is what recon_line_pool_ragged_*
 * takes).  The cells of a row are those of the same line in recon_ctx_batch_fill's arrays; every cell of the L rows is written exactly
 * once, as runs of 16-byte stores, and nothing behind row L.  RECON_ERR_INVALID unless U <= L <= U P_b.  Two launches. */
int recon_ctx_batch_fill_ragged(const void* const* tables, const int64_t* dims, const int64_t* unique_entities, const int32_t* unique_info,
                                int64_t U, int64_t L, int32_t P_b, int32_t T_b, int32_t index_bytes, void* context_words, void* context_chars,
                                int32_t* line_ptr, int32_t* row_entity, recon_stream_t stream);
/* get_gat_entity_embeddings / get_selected_gat_entity_embeddings (train.py:250-258; utils/context_utils.py:444-475):
 * gat_entity_embeddings fp32 [n_pairs][2 G] = (gat_emb[gat_row[head]] | gat_emb[gat_row[tail]]), a zero half for a row below 0; with
 * nonzero_gat_entity_embeddings [Mnz][2 G] (optional) the same row again at pair_slot[pair] >= 0.  Any G >= 1.  One launch. */
int recon_ctx_batch_gat(const void* const* tables, const int64_t* dims, const int64_t* entity_indices, int64_t n_pairs, const int32_t* pair_slot,
                        float* gat_entity_embeddings, float* nonzero_gat_entity_embeddings, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * E15  A stage-B iteration's two ends over a device-resident dataset (csrc/stage_b.hip; recon_amd/stage_b.py): the batch's rows of the
 *      arrays that graphs_to_indices returns (parsing/legacy_sp_models.py:276-333), and the rows of a test pass's result file.
 *      Selection and copying only: integers to the value, confidence to the bit.  Every entry: RECON_ERR_INVALID for a NULL pointer, a
 *      count or M below 1 or a range outside its array, RECON_ERR_UNSUPPORTED above recon_stage_b_supported's limit, both before any
 *      launch.  No allocation, no workspace, no atomics, bitwise reproducible.
 * ------------------------------------------------------------------------------------------*/
/* 1 when a batch of `count` sentences with num_pairs = n (n - 1) entity pairs and sent_len tokens runs in recon_stage_b_slice
 * (train.py:247-251): every extent at least 1 and the largest output — entity_markers [count][num_pairs][sent_len], or the id pairs
 * [count][num_pairs][2] — below 2^31 - 4096 cells (flat output indices are int32).  The reference's batch is 50 x 72 x 36. */
int recon_stage_b_supported(int64_t count, int64_t num_pairs, int64_t sent_len);
/* train.py:247-251 with the casts of :261-262 and :309 (again :333-337, and test.py), one launch: batch row b is dataset row
 * r(b) = order[start + b] (order NULL: start + b), order int64 [order_len] with start + count <= order_len (order NULL: <= N).  A value
 * of `order` is CLAMPED into [0, N) before use and never becomes an address; validating it is the host's part.  Reads sentences int32
 * [N][sent_len], markers int8 [N][num_pairs][sent_len], labels int16 [N][num_pairs], num_entities int32 [N] and, both or neither of a
 * pair, entity_indices / surface_ids int32 [N][num_pairs][2] with their outputs.  Writes sentence_input [count][sent_len] and
 * entity_markers [count][num_pairs][sent_len] of index_bytes = 4 or 8 (int32 / int64), labels_out int64 [count num_pairs] row-major,
 * num_entities_out int32 [count], entity_indices_out int64 [count][num_pairs][2] (sign-extended: -1 stays -1), surface_ids_out int32
 * [count][num_pairs][2] and rows_out int64 [count] = r(b).  Every cell is written exactly once, as runs of 16-byte stores (element
 * stores at an unaligned array's two ends). */
int recon_stage_b_slice(const int32_t* sentences, const int8_t* markers, const int16_t* labels, const int32_t* num_entities,
                        const int32_t* entity_indices, const int32_t* surface_ids, int64_t N, int64_t num_pairs, int64_t sent_len,
                        const int64_t* order, int64_t order_len, int64_t start, int64_t count, int32_t index_bytes, void* sentence_input,
                        void* entity_markers, int64_t* labels_out, int32_t* num_entities_out, int64_t* entity_indices_out,
                        int32_t* surface_ids_out, int64_t* rows_out, recon_stream_t stream);
/* test.py:285-292 and the indices of :300-302, one launch of one workgroup: for every m < M with labels[m] != ignore_index, in row order,
 * appends (rows[m / num_pairs] num_pairs + m % num_pairs, predicted[m], labels[m], confidence[m]) to the four output arrays of
 * `capacity` elements, starting at state[0].  labels, predicted int64 [M], confidence fp32 [M], rows int64 [M / num_pairs] (M a multiple
 * of num_pairs).  state int64 [2] on the device: [0] the count of rows appended so far, read at the start and stored at the end with
 * plain loads and stores — the calls that share a state must run on ONE stream; [1] set to 1 when a row's place was at or beyond
 * `capacity`: such a row is not stored, the count goes on.  The outputs may be NULL when capacity is 0. */
int recon_stage_b_collect(const int64_t* labels, const int64_t* predicted, const float* confidence, const int64_t* rows, int64_t M,
                          int64_t num_pairs, int64_t ignore_index, int64_t* state, int64_t capacity, int64_t* out_pair,
                          int64_t* out_predicted, int64_t* out_gold, float* out_confidence, recon_stream_t stream);
/* 1 when a batch of `count` rows of the per-pair baselines' datasets (one entity pair per row; marker_rows 1: LSTM's markers [N][sent_len],
 * 2: the relative positions [N][2][sent_len] of CNN and PCNN) runs in recon_pair_slice: every extent at least 1 and the largest output —
 * the mask [count][3][sent_len]; the bound is the same without one — below 2^31 - 4096 cells.  The reference's batch is 50 x 36. */
int recon_pair_slice_supported(int64_t count, int64_t marker_rows, int64_t sent_len);
/* train.py:247-249 with the casts of :301-309 (again :333-335, :387-393) over what parsing/legacy_sp_models.py:67-97 and :503-603 return, one launch of
 * k_sb_slice's scheme: batch row b is dataset row r(b) = order[start + b] (order NULL: start + b), CLAMPED into [0, N) as in
 * recon_stage_b_slice, whose range rules hold.  Reads sentences int32 [N][sent_len], markers int8 [N][marker_rows][sent_len], labels int16
 * [N] and, with pcnn_mask or not at all, segment_bits uint8 [N][sent_len]: bit s of byte [n][t] is the reference's pcnn_mask[n][s][t].
 * Writes sentence_input [count][sent_len] and entity_markers [count][marker_rows][sent_len] of index_bytes = 4 or 8, sign-extended,
 * pcnn_mask fp32 [count][3][sent_len] = ((segment_bits[r(b)][t] >> s) & 1) as 0.0f / 1.0f, labels_out int64 [count] and rows_out int64
 * [count] = r(b).  The mask follows `order` like every other array (train.py:304 takes it from the unshuffled rows).  Every cell is
 * written exactly once, as runs of 16-byte stores (element stores at an unaligned array's two ends). */
int recon_pair_slice(const int32_t* sentences, const int8_t* markers, const int16_t* labels, const uint8_t* segment_bits, int64_t N,
                     int64_t marker_rows, int64_t sent_len, const int64_t* order, int64_t order_len, int64_t start, int64_t count,
                     int32_t index_bytes, void* sentence_input, void* entity_markers, float* pcnn_mask, int64_t* labels_out, int64_t* rows_out,
                     recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * E16 ContextAware's attention over ghosts (csrc/pair_attn.hip): the per-sentence self-attention over the pair states with the diagonal
 *     left out, between the encoder and the head of the baseline model (models/baselines.py:86-112):
 *     S[b][i][j] = memory[b][i] . states[b][j] for j != i;  P[b][i][:] = softmax over j != i of S[b][i][:], P[b][i][i] = 0;
 *     out[b][i] = (states[b][i] | sum_j P[b][i][j] states[b][j])                                                    [B][C][2 D]
 *     states and memory (= states W^T: recon_pair_transitions_fwd with act linear and no bias forms it) are B C rows of D floats at
 *     ONE row stride each (ld_s, ld_m >= D, elements), sentence b's pair i at row b C + i; out and g_out B C rows of 2 D floats at the
 *     row strides ld_out, ld_g >= 2 D; P, g_states, g_memory and the workspace contiguous; all fp32.  Every pair attends over all the
 *     others of its sentence, padding pairs included: there is no mask.  C == 1: P = 0, the right half of out is zero and nothing flows
 *     through it.  Non-finite inputs are outside the contract: a NaN or an infinity in a row of scores gives NaN in that row's P.
 *     Everything is fp32 on v_mfma_f32_16x16x4_f32, without atomics, every sum in an order the shape alone decides, every output cell
 *     written exactly once by ordinary vector stores: bitwise identical from run to run.  Status codes and the 16-byte alignment of
 *     workspace are those of the E8 - E12 entries; nothing is allocated inside the library.
 * ------------------------------------------------------------------------------------------*/
/* Shapes the kernels take (models/baselines.py:86-112): B >= 0, 1 <= C <= 160 pairs (n <= 13 entities), D a multiple of 4 in 4..1024,
 * B C <= 2^24.  The fwd / bwd entries also need 16-byte aligned states, memory, out and g_out and row strides that are multiples of 4.
 * Everything else answers RECON_ERR_UNSUPPORTED and writes nothing; the caller then runs the stock ops. */
int recon_pair_attention_supported(int64_t B, int32_t C, int32_t D);
/* Bytes of the workspace (models/baselines.py:86-112).  Forward (backward = 0): none.  Backward (backward = 1): g_S, B C C floats.
 * 16-byte aligned, any contents; 0 for a shape recon_pair_attention_supported refuses and for B == 0. */
size_t recon_pair_attention_workspace_bytes(int64_t B, int32_t C, int32_t D, int32_t backward);
/* Forward (models/baselines.py:86-112), one launch: workgroup (sentence, tile of 16 target pairs) forms its 16 x C scores over D, the
 * row softmax and its 16 rows of out, both halves (no cat is written).  P [B][C][C] or NULL (no backward will follow: it is not stored).
 * B == 0: nothing is launched. */
int recon_pair_attention_fwd(const float* states, int64_t ld_s, const float* memory, int64_t ld_m, int64_t B, int32_t C, int32_t D, float* out,
                             int64_t ld_out, float* P, recon_stream_t stream);
/* Backward (models/baselines.py:86-112) from g_out = (g_left | g_ctx), read in place; it destroys nothing (any number of backwards per
 * forward, the same bits each time).  T[i][j] = g_ctx[i] . states[j], r[i] = sum_j P[i][j] T[i][j], g_S = P (T - r) into the workspace
 * (first launch, workgroup (sentence, 16-row tile)); then workgroup (sentence, 64 columns of D) writes
 * g_memory[:, chunk] = g_S states[:, chunk] and g_states[:, chunk] = g_left + (P^T g_ctx[:, chunk] + g_S^T memory[:, chunk]), each
 * reduction over the pairs ascending.  g_states, g_memory [B][C][D] or NULL (not wanted: its passes are skipped; both NULL: nothing is
 * launched).  g_states lacks the part through memory: that is recon_pair_transitions_bwd's d_x over g_memory.  B == 0: nothing is
 * launched.  Two launches. */
int recon_pair_attention_bwd(const float* states, int64_t ld_s, const float* memory, int64_t ld_m, const float* P, const float* g_out,
                             int64_t ld_g, int64_t B, int32_t C, int32_t D, float* g_states, float* g_memory, void* workspace,
                             size_t workspace_bytes, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * E17 The sentence convolution and pool of the per-pair baselines CNN and PCNN (csrc/sent_conv.hip; models/baselines.py:237-247 and
 *     :297-308): the three embedding gathers, the dropout product, cat, transpose, the Conv1d's, the max over the positions, the pooled
 *     dropout and the activation.  Cin = Dw + 2 Dp:
 *     x[b][t]         = (keep . word_table[sentence[b][t]] | pos_table_0[positions[b][0][t]] | pos_table_1[positions[b][1][t]])
 *     conv_i[b][e][t] = bias_i[e] + sum_j sum_c w_i[e][c][j] x[b][t + j - pad_i][c],  x zero outside 0..T-1
 *     segments NULL (CNN):  pad_i = 0, T_out = T - k_i + 1, pooled[b][i E + e] = max_t conv_i[b][e][t]
 *     segments [B][3][T] (PCNN): n == 1, k odd, pad = k / 2, T_out = T, pooled[b][s E + e] = max_t conv[b][e][t] segments[b][s][t], a
 *                           product: a position whose factor is 0 contributes exactly 0
 *     out[b][:]       = act(pool_keep . pooled[b][:])        [B][n_out E], n_out = n (CNN) or 3 (PCNN); act 0 none, 1 tanh, 2 relu
 *     An exact tie takes the lowest position.  max_at [B][n_out E] is one byte per output: the winning position, or 255 when the maximum
 *     was the 0 of a zero-factor position (no gradient).  sentence [B][T] of sentence_bytes 4 or 8 (int32 / int64), positions [B][2][T]
 *     of position_bytes 1, 4 or 8, both contiguous; word_table [V][Dw], pos_table_0/1 [P][Dp], weights[i] [E][Cin][k_i] (nn.Conv1d's
 *     layout), biases[i] [E], ks[i] = k_i: `weights`, `biases`, `ks` and the g_ arrays are HOST arrays of n entries.  keep: at most one
 *     of keep_bits (uint32 [B][T][ceil(Dw / 32)], factor = keep_scale where bit c % 32 of word c / 32 is set, else 0) and keep_factors
 *     (fp32 [B][T][Dw]); pool_keep fp32 [B][n_out E] or NULL.  An id outside its table is never used as an address: row 0 is read in its
 *     place and status[0] (device int32, zeroed by the caller) is set to 1.  x, its transpose, the convolution outputs and their masked
 *     copies are never written.  fp32 on v_mfma_f32_16x16x4_f32 (forward) and the VALU (backward), no atomics, every sum in an order the
 *     shape alone decides, every output cell written exactly once by ordinary vector stores.  Status codes and the 16-byte alignment of
 *     workspace are those of the E8 - E16 entries; nothing is allocated inside the library.
 * ------------------------------------------------------------------------------------------*/
/* Shapes the kernels take (models/baselines.py:237-247, :297-308): 0 <= B <= 2^24, 1 <= T <= 128, Cin = Dw + 2 Dp <= 320, E <= 1024,
 * 1 <= n <= 4 weights of 1 <= k_i <= 9, 2 P Dp <= 4096 and 2 T Dp <= 4096 (the position-table slabs of the backward).  T_out <= 128 is
 * within the byte's 255.  RECON_ERR_INVALID shapes (k_i > T without segments; with segments n != 1 or an even k) answer 0 as well. */
int recon_sent_conv_supported(int64_t B, int32_t T, int32_t Dw, int32_t Dp, int32_t P, int32_t E, const int32_t* ks, int32_t n,
                              int32_t segmented);
/* Bytes of the workspace (models/baselines.py:237-247, :297-308).  Forward (backward = 0): the weights K-major, sum_i
 * ceil(Cin / 100 chunks) k_i pitch (E rounded up to 16) floats.  Backward: G slabs of (d_w | d_bias), G = min(32, B, 2^24 floats / slab),
 * and min(256, B) slabs [2][P][Dp] of the position tables: bounded independently of B.  0 for a refused shape and for B == 0. */
size_t recon_sent_conv_workspace_bytes(int64_t B, int32_t T, int32_t Dw, int32_t Dp, int32_t P, int32_t E, const int32_t* ks, int32_t n,
                                       int32_t segmented, int32_t backward);
/* Forward (models/baselines.py:237-247, :297-308), two launches: the weights K-major into the workspace; then workgroup (rows, 64 output
 * channels, weight) stages its rows' gathered x in LDS, multiplies and pools.  max_at may be NULL (no backward will follow).  B == 0:
 * nothing is launched. */
int recon_sent_conv_fwd(const void* sentence, int32_t sentence_bytes, const void* positions, int32_t position_bytes, const float* word_table,
                        int32_t V, const float* pos_table_0, const float* pos_table_1, int32_t P, const void* keep_bits, float keep_scale,
                        const float* keep_factors, const float* segments, const void* const* weights, const void* const* biases,
                        const int32_t* ks, int32_t n, const float* pool_keep, int32_t activation, int64_t B, int32_t T, int32_t Dw, int32_t Dp,
                        int32_t E, float* out, void* max_at, int32_t* status, void* workspace, size_t workspace_bytes, recon_stream_t stream);
/* Backward (models/baselines.py:237-247, :297-308) from g_out [B][n_out E], out and max_at; it destroys nothing (any number of backwards
 * per forward, the same bits each time).  g = g_out act'(out) pool_keep f, f the segment factor at the winning position; x is gathered
 * again.  d_w_i[e][c][j] = sum_b g x[b][t* + j - pad][c], d_bias_i[e] = sum_b g, rows ascending inside a group, groups ascending;
 * d_pos_table_h[p] = sum over (b, t) with positions[b][h][t] = p of d_x[b][t][its columns], row pos_padding_idx (-1: none) left zero.
 * Any g_ pointer (or entry of g_weights / g_biases, or either array) may be NULL: not wanted; nothing wanted: nothing is launched.  At
 * most three launches.  B == 0: zeros in every wanted gradient. */
int recon_sent_conv_bwd(const void* sentence, int32_t sentence_bytes, const void* positions, int32_t position_bytes, const float* word_table,
                        int32_t V, const float* pos_table_0, const float* pos_table_1, int32_t P, const void* keep_bits, float keep_scale,
                        const float* keep_factors, const float* segments, const void* const* weights, const int32_t* ks, int32_t n,
                        const float* pool_keep, int32_t activation, int64_t B, int32_t T, int32_t Dw, int32_t Dp, int32_t E, const float* out,
                        const void* max_at, const float* g_out, int32_t pos_padding_idx, float* g_pos_table_0, float* g_pos_table_1,
                        void* const* g_weights, void* const* g_biases, void* workspace, size_t workspace_bytes, recon_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * E18 The distinct (sentence, pair markers) sequences of a stage-B batch (csrc/pair_groups.hip; recon_amd/pair_groups.py).
 *     to_indices_with_real_entities_and_entity_nums_with_vertex_padding (parsing/legacy_sp_models.py:294-326) fills
 *     entity_matrix[index, new_j] only for the edges a sentence has, every other pair slot keeps an all-zero marker row, and GPGNN.encode
 *     (models/models.py:160-184) copies the sentence once per slot: the slots of a sentence whose marker rows are equal are one LSTM
 *     input.  Grouping rule: two pair slots of the SAME sentence share a sequence exactly when their marker rows are equal element by
 *     element (not "all zero"); slots of different sentences never share.  The representative of a group is its lowest c, and the S_d
 *     distinct sequences are numbered in (b, lowest c) order.  Selection, ordering and copying only; no global atomics, no hash, bitwise
 *     reproducible; every index read back from memory is clamped before it is used as an address.  Status codes are those of the
 *     E8 - E17 entries; nothing is allocated inside the library.
 * ------------------------------------------------------------------------------------------*/
/* 1 when markers [B][C][T] (parsing/legacy_sp_models.py:294-326) are grouped by the kernels: 1 <= B <= 8192 sentences per call,
 * 1 <= C <= 256 pair slots, T >= 1 and B C T below 2^31 - 4096.  The reference's batch is 50 x 72 x 36. */
int recon_pair_groups_supported(int64_t B, int64_t C, int64_t T);
/* Bytes of recon_pair_groups_build's workspace (parsing/legacy_sp_models.py:294-326): first and local_rank int32 [B C] and counts
 * int32 [B]; 16-byte aligned, any contents; 0 for a refused shape. */
size_t recon_pair_groups_workspace_bytes(int64_t B, int64_t C, int64_t T);
/* The grouping inside each sentence (parsing/legacy_sp_models.py:294-326; models/models.py:160-184), one launch, one workgroup per
 * sentence: markers [B][C][T] contiguous, of marker_bytes 1, 4 or 8 (int8 as the resident dataset stores them, int32, int64), compared
 * exactly, word-wise, every row against the rows in front of it.  Writes first int32 [B C] (the lowest c' of the sentence whose row
 * equals slot c's), local_rank int32 [B C] (the number of the slot's group among the sentence's groups, in lowest-c order) and counts
 * int32 [B] (the sentence's distinct rows). */
int recon_pair_groups_local(const void* markers, int32_t marker_bytes, int64_t B, int64_t C, int64_t T, int32_t* first, int32_t* local_rank,
                            int32_t* counts, recon_stream_t stream);
/* The maps of a batch (parsing/legacy_sp_models.py:294-326; models/models.py:160-184), two launches: recon_pair_groups_local into the
 * workspace, then ONE workgroup scans counts in b order into seq_ptr int32 [B + 1] and writes pair_seq int32 [B C] (the sequence of every
 * pair), seq_pair int32 [total] (the flat pair index b C + c of every sequence's representative) and the rows the encoder reads,
 * sentence_d [total][T] and markers_d [total][T] of index_bytes 4 or 8: the representatives' rows of sentence [B][T] (index_bytes wide)
 * and of markers.  `total` is the caller's S_d (B <= total <= B C, else RECON_ERR_INVALID): when the scan finds another one, status[0]
 * (device int32, zeroed by the caller) is set to 1, pair_seq is clamped below total, rows between the two totals are zeros and nothing
 * is written at or behind row total.  total < 0: seq_ptr and pair_seq alone (seq_ptr[B] is S_d; the other outputs may be NULL). */
int recon_pair_groups_build(const void* sentence, int32_t index_bytes, const void* markers, int32_t marker_bytes, int64_t B, int64_t C, int64_t T,
                            int64_t total, int32_t* seq_pair, int32_t* pair_seq, int32_t* seq_ptr, void* sentence_d, void* markers_d, int32_t* status,
                            void* workspace, size_t workspace_bytes, recon_stream_t stream);
/* out [n_pairs][F] = rows[pair_seq[p]][:] (models/models.py:160-184: every pair slot's state from its sequence's), fp32, one launch of
 * 16-byte stores (element stores where F is no multiple of 4 or a base is not 16-byte aligned).  pair_seq is clamped into [0, S_d).
 * n_pairs F and S_d F below 2^31 - 4096.  n_pairs == 0: nothing is launched. */
int recon_pair_groups_expand(const float* rows, const int32_t* pair_seq, int64_t n_pairs, int64_t S_d, int32_t F, float* out, recon_stream_t stream);
/* The backward of recon_pair_groups_expand (models/models.py:160-184), one launch: g_rows[j][:] = the sum of g_out[b C + c][:] over the
 * slots c of sequence j's sentence b = seq_pair[j] / C with pair_seq[b C + c] == j, c ascending: one fp32 chain per element, one wave per
 * (sequence, chunk of columns), no atomics; it destroys nothing (any number of backwards per forward, the same bits each time).
 * S_d == 0: nothing is launched. */
int recon_pair_groups_reduce(const float* g_out, const int32_t* pair_seq, const int32_t* seq_pair, int64_t B, int64_t C, int64_t S_d, int32_t F,
                             float* g_rows, recon_stream_t stream);

/* ---- E19: the distinct word forms of an entity-context batch (recon_amd/word_forms.py, csrc/word_forms.hip, csrc/ctx_batch.hip) ----------
 * `get_char_indices` (utils/context_utils.py:265-283) lays every word slot of a context line out as [cfs - 1 pads][max_char_len ids]
 * [cfs - 1 pads], and the char-CNN (models/models.py:57-61) computes a slot's feature from that window alone: it is run once per distinct
 * window (a form) and the feature rows are copied to the forms' slots (recon_pair_groups_expand with slot_form as the map). */
/* Slots per piece of the backward below (models/models.py:57-61; a constant of the build). */
int32_t recon_word_forms_piece(void);
/* Scratch of recon_word_forms_reduce (models/models.py:57-61): (n_slots / piece + S_d + 1) F floats; 0 for a shape it refuses. */
size_t recon_word_forms_reduce_workspace_bytes(int64_t n_slots, int64_t S_d, int32_t F);
/* The backward of the copy (models/models.py:57-61: the gradient of a form's feature row is the sum of its slots'), two launches:
 * g_rows[f][:] = the sum of g_out[s][:] over s = form_slots[form_ptr[f] .. form_ptr[f + 1]) in list order, fp32.  form_ptr int32
 * [S_d + 1], form_slots int32 [n_slots] (the slots of form 0, then of form 1, ...).  A segment is cut into pieces of
 * recon_word_forms_piece() slots from ITS start; a piece is one fp32 chain per element, and a form's pieces are added in piece order: the
 * result depends on a form's own list alone, is the same bits from run to run, and nothing is destroyed.  A form without a slot gets
 * zeros.  form_ptr and form_slots are clamped into [0, n_slots] and [0, n_slots) before use.  n_slots F, S_d F and the scratch below
 * 2^31 - 4096 floats.  S_d == 0: nothing is launched. */
int recon_word_forms_reduce(const float* g_out, const int32_t* form_ptr, const int32_t* form_slots, int64_t n_slots, int64_t S_d, int32_t F, float* g_rows,
                            void* workspace, size_t workspace_bytes, recon_stream_t stream);
/* Scratch of the two entries below (utils/context_utils.py:265-283): 3 num_forms int32 (flags, ranks, the list of present forms); 0 for a num_forms they refuse. */
size_t recon_ctx_batch_forms_scratch_bytes(int64_t num_forms);
/* Between recon_ctx_batch_index and the host's read of the header (utils/context_utils.py:265-283 under :365-385): which of the tables'
 * num_forms word forms the batch holds.  tok_form int32 [V] is every token's form (form 0: the all-pad window of an empty word slot),
 * form_chars int32 [num_forms][max_char_len] the forms' char ids.  Three launches on `stream`: the flags are cleared, every token of
 * every line of the batch stores 1 into its form's flag (and a line shorter than T_b into form 0's; the sizes are read from the header
 * on the device; ragged = 1: the padding lines do not exist), and one workgroup scans the flags: the batch numbers its forms by ascending
 * table form.  header[7] = S_d.  tables and dims are recon_ctx_batch_index's; n_pairs bounds the entities walked. */
int recon_ctx_batch_forms_count(const void* const* tables, const int64_t* dims, const int32_t* tok_form, const int32_t* form_chars, int64_t num_forms,
                                const int64_t* unique_entities, const int32_t* unique_info, int64_t n_pairs, int32_t ragged, int32_t* scratch,
                                int32_t* header, recon_stream_t stream);
/* recon_ctx_batch_fill (ragged = 0: n_rows = U P_b and context_mask; line_ptr and row_entity unused) or recon_ctx_batch_fill_ragged
 * (ragged = 1: n_rows = L, line_ptr and row_entity; context_mask unused) with the char block as its distinct windows
 * (utils/context_utils.py:265-283): form_rows [S_d][2 (cfs - 1) + max_char_len] of index_bytes, one `W = 1` row of
 * recon_char_features_fwd per form, and slot_form int32 [n_rows T_b], the form of every word slot.  The dense [n_rows][W] block is not
 * written.  scratch is what recon_ctx_batch_forms_count left for this batch, S_d the header's eighth word. */
int recon_ctx_batch_fill_forms(const void* const* tables, const int64_t* dims, const int32_t* tok_form, const int32_t* form_chars, int64_t num_forms,
                               const int32_t* scratch, const int64_t* unique_entities, const int32_t* unique_info, int64_t U, int64_t n_rows, int32_t P_b,
                               int32_t T_b, int64_t S_d, int32_t ragged, int32_t index_bytes, void* context_words, void* context_mask, int32_t* line_ptr,
                               int32_t* row_entity, void* form_rows, int32_t* slot_form, recon_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECON_HIP_H */
