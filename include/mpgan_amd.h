/* mpgan_amd.h -- C ABI of libmpgan_amd.so (MI355X / gfx950 hot path of MPGAN + GAPT).
 *
 * Plain pointers and sizes only: every pointer is a DEVICE pointer into caller-owned fp32
 * (or, where noted, packed-bf16 "image") memory, `stream` is a hipStream_t passed as
 * void*, and every entry point enqueues work on that stream and returns at once
 * (0 = success, otherwise a hipError_t value or a negative argument-error code).  Nothing
 * is allocated, freed or synchronised inside, so every call can be captured in a hipGraph.
 *
 * The reference (rkansal47/MPGAN) has no FFI: its hot path is Python calling ATen.  Each
 * entry point below therefore cites the reference Python lines whose ATen work it replaces
 * (paths relative to the reference root); INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 */
#ifndef MPGAN_AMD_H
#define MPGAN_AMD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- generic fused linear (nn.Linear + LeakyReLU + Dropout and their backward) -----------
 * Replaces LinearNet.forward's per-layer addmm / leaky_relu / dropout (mpgan/model.py:77-83,
 * gapt/model.py:78-84) and their autograd backward for the node network fn, the final fnd
 * layer and GAPT's projections. */
typedef struct MpgGemm {
    const float* A;      /* A(m,k) = ak ? A[m*lda+k] : A[k*lda+m]                                   */
    const float* A2;     /* optional second K-segment: columns k >= K1 come from A2(m, k-K1) (ak=1) */
    int lda, lda2, K1;
    const float* B;      /* B(k,n) = bk ? B[n*ldb+k] : B[k*ldb+n]                                   */
    int ldb;
    float* C;            /* C[m*ldc+n]; with split-K, slice z is written at C + z*split_stride      */
    int ldc;
    int M, N, K;
    long long split_stride;
    const float* bias;   /* [N] or NULL                                                             */
    float out_scale;     /* product is multiplied by this before the bias                           */
    int act;             /* 1 = LeakyReLU(alpha)                                                    */
    float alpha;
    const uint64_t* seed;/* device pointer to the 64-bit dropout seed (NULL = no dropout anywhere)  */
    uint32_t drop_tag, drop_thr; float drop_scale;   /* forward dropout on C (thr = round(256 p))   */
    const float* gateH;  /* backward: C *= d(dropout o act)/dz evaluated from the saved output H    */
    int ldh, gate_act;
    uint32_t gate_tag, gate_thr; float gate_scale;
    const float* resid;  /* C += resid[m*ldr+n]                                                     */
    int ldr;
    int accumulate;      /* C += result instead of C = result                                       */
    int f16;             /* 1: split operands as fp16 hi/lo (forward products); 0: bf16 hi/lo (gradients);
                          * 2 (mpg_gemm_wgrad_group only, every job of the call): one-term fp16 products on 128 x 128 tiles with a
                          * power-of-two unit per 128 rows of A -- needs 16-byte aligned B, ldb % 4 == 0 and rows of B at least
                          * as long as their width rounded up to 4 (-3 otherwise)                                     */
    int ones_col;        /* 1: column N-1 of B is the constant 1 (N counts it): C[:, N-1] = row sums of A  */
} MpgGemm;

int mpg_gemm(const MpgGemm* g, int ak, int bk, int splitk, void* stream);

/* Sum S split-K partial slices [S][N][K + has_bias] into out[n*ldo + k] (and bias[n] from the extra column). */
int mpg_splitk_reduce(const float* part, int S, int N, int K, int has_bias, float* out, int ldo, float* bias,
                      void* stream);

/* Several weight-gradient GEMMs (dW = dY^T X: AK = BK = 0, split-K partials) / their split-K reductions in ONE
 * launch each: the six weight gradients of an MPLayer are each too small to fill the chip on their own. */
#define MPG_GROUP_MAX 16
typedef struct MpgReduceJob {
    const float* part; int S, N, K, has_bias; float* out; int ldo; float* bias;
    int accumulate;      /* add to out / bias instead of overwriting (gradient accumulation into .grad) */
} MpgReduceJob;
int mpg_gemm_wgrad_group(const MpgGemm* g, const int* splitk, int n, void* stream);
int mpg_splitk_reduce_group(const MpgReduceJob* jobs, int n, void* stream);

/* out = in * gate(H): backward through Dropout (and LeakyReLU when gate_act) ahead of a GEMM. */
int mpg_gate(const float* in, int ldi, const float* H, int ldh, float* out, int ldo, int M, int N,
             int gate_act, float alpha, const uint64_t* seed, uint32_t tag, uint32_t thr, float scale,
             void* stream);

/* mpg_slab_sums: out[m, 0:cols] = sum_s A[s][m][0:cols], out[m, cols:2 cols] = sum_s B[s][m][0:cols] (slab s at A + s * strideA
 * floats, rows dense; added in index order).  The partial receiver gradients da (one slab per sender chunk) and sender gradients dc
 * (one slab per receiver block) of a sender-chunked mpg_edge_bwd launch, as the [da | dc] rows the layer's dx chain and its first
 * layer's weight gradient read -- replaces the two `sum(0)` calls autograd would issue for the reference's
 * `A.view(B, N, N, -1).sum(2)` backward (mpgan/model.py:257-267).  cols % 4 == 0, 16-byte aligned pointers (-5). */
int mpg_slab_sums(const float* A, int slabsA, uint64_t strideA, const float* B, int slabsB, uint64_t strideB,
                  float* out, int M, int cols, void* stream);

/* Test helper: the {0,1} keep mask [rows, F] the kernels use for dropout site `tag`. */
int mpg_dropout_mask(float* out, uint64_t rows, int F, const uint64_t* seed, uint32_t tag, uint32_t thr,
                     void* stream);

/* ---- fused edge network of MPLayer ------------------------------------------------------------
 * Widths are the reference defaults fe = [96,160,192] (setup_training.py:471-477).
 *
 * mpg_pack_weights: W[rows,cols] (row stride ldw; transpose=1 reads W^T) * scale  ->  bf16 hi/lo
 * (f16=0) or fp16 hi/lo (f16=1)
 * fragment image of ceil(rows/32) x ceil(cols/32) x 2 fragments of 1 KiB, hi part then lo part
 * (2 * MT*QT*2 KiB in all).  Layer images: W2 = fe.net.1.weight (160x96), W3 = fe.net.2.weight
 * (192x160); the backward also takes their transposes.  When dropout is on, `scale` carries the
 * 1/(1-p) of the dropout in FRONT of that layer (inverted dropout commutes with LeakyReLU). */
int mpg_pack_weights(const float* W, int ldw, int rows, int cols, int transpose, float scale, int f16,
                     void* img, void* stream);

/* mpg_pack_many: up to MPG_PACK_MAX_JOBS images in one launch (all images of a layer after an optimizer step).
 * rows/cols are those of the PACKED matrix, which is W (transpose = 0) or W^T (transpose = 1).  row_split > 0
 * reads a stacked view of W: logical row n of the un-transposed matrix is W[n % row_split, (n / row_split) *
 * split_cols + col] -- fe.net.0.weight [96, 2F] seen as [a-half ; c-half] = [192, F]. */
#define MPG_PACK_MAX_JOBS 24
typedef struct MpgPackJob {
    const float* W; int ldw, rows, cols, transpose; float scale; int f16; void* img;
    int row_split, split_cols;
    int* status;   /* optional device word, OR-ed into: 1 = an element of an fp16 image is beyond fp16's range after scaling
                      (|W * scale| > 65504: the image holds inf and every product with it is lost), 2 = a weight is not finite */
} MpgPackJob;
int mpg_pack_many(const MpgPackJob* jobs, int njobs, void* stream);

/* mpg_chain: up to three Linear(+LeakyReLU)(+Dropout) layers -- or their input-gradient chain -- on row blocks
 * of 32 without the intermediates returning to memory as operands.  Replaces LinearNet.forward
 * (mpgan/model.py:70-85) for MPLayer.fn (:268-279) and, in its backward, the three dX = dY W products.
 *   layer l:  z = Wimg_l x + bias ;  y = z                      (act = 0)
 *                                    y = LeakyReLU(z)            (act = 1)
 *             y = dropout(y)  (drop_thr != 0: keep * drop_scale) ; y *= gate(H)  (gateH != NULL: derivative of
 *             Dropout o LeakyReLU [gate_act] of the forward layer whose OUTPUT is H, as mpg_gemm's gate) ;
 *             y += resid (resid != NULL)
 *   input  :  rows of A (sum of a_slabs slabs, K1 columns) followed by rows of A2 (K - K1 columns); in_thr != 0
 *             multiplies it by a dropout keep mask first (backward of a trailing dropout) and in_out, if given,
 *             receives that gated input.
 * Wimg_l is the mpg_pack_weights image of the [N, K] matrix applied (the transposed weight in the backward),
 * fp16 hi/lo when f16 else bf16 hi/lo.  K, N <= 256 for every layer but the last (N unbounded there).
 * wscale / ascale: exact power-of-two operand scales that keep the lo halves of fp16 pairs out of the subnormal
 * range (an fp16 hi/lo pair has its 22 bits only for |x| >= 2^-3); results are unscaled before the epilogue. */
typedef struct MpgChainLayer {
    const void* Wimg; const float* bias; int nbias;      /* bias[n] for n < nbias, 0 beyond (nbias = 0: all N) */
    int K, N, act;
    uint32_t drop_tag, drop_thr; float drop_scale;
    const float* gateH; int ldh, gate_act;
    uint32_t gate_tag, gate_thr; float gate_scale;
    const float* resid; int ldr;                         /* y += resid[m, n] (after everything else), or NULL */
    float* out; int ldo;
    float wscale;                                        /* the image holds wscale * W (a power of two; 0 = 1): z is divided by it */
} MpgChainLayer;
typedef struct MpgChain {
    const float* A; int lda, K1;
    const float* A2; int lda2;
    int a_slabs; uint64_t a_slab_stride;
    uint32_t in_tag, in_thr; float in_scale;
    float* in_out; int ld_in_out;
    int M, nlayers; float alpha; const uint64_t* seed; int f16;
    float ascale;                                        /* activations are split as ascale * x (a power of two; 0 = 1) */
    MpgChainLayer L[3];
} MpgChain;
int mpg_chain(const MpgChain* p, void* stream);
/* mpg_chain_route: which kernel mpg_chain would run for `p`, without launching anything (host only: struct fields and
 * pointer VALUES are read, nothing is dereferenced).  The checks are mpg_chain's own, in its order -- mpg_chain decides
 * through this function -- so a refusal returns mpg_chain's negative code; otherwise one of
 *   MPG_CHAIN_ROUTE_CHAIN2    the fixed shape table of chain2.hip (the MPLayer shapes),
 *   MPG_CHAIN_ROUTE_STRAIGHT  the general kernel of chain.hip, one of its instantiations with straight-line k loops
 *                             (the same k-steps as the MPLayer shapes: what MPG_CHAIN_GENERAL=1 in the environment,
 *                             read on every call, sends them to),
 *   MPG_CHAIN_ROUTE_LOOPS     the general kernel with run-time k loops (every other shape). */
#define MPG_CHAIN_ROUTE_CHAIN2 1
#define MPG_CHAIN_ROUTE_STRAIGHT 2
#define MPG_CHAIN_ROUTE_LOOPS 3
int mpg_chain_route(const MpgChain* p);

/* mpg_edge_fwd: replaces MPLayer._getA_fully_connected + self.fe(A) + mask multiply + sum/mean
 * (mpgan/model.py:241, :256-267, :284-317).  Inputs are the layer-1 node terms
 *   a[b,i,:] = W1[:, :F] x_i + b1   (receiver),   c[b,j,:] = W1[:, F:] x_j   (sender),
 * so that fe.net.0 applied to [x_i ; x_j] is a_i + c_j exactly.  Output
 *   agg[b,i,:] = agg_scale * sum_j mask[b,j] * fe([x_i ; x_j])        ([B,N,192], agg_scale = 1 | 1/N)
 * With SC > 1 the senders are split over SC workgroups and agg has a leading [SC] axis of partial
 * sums the caller adds up (mpg_edge_fwd_fn with `tickets` adds them up itself: the last workgroup to arrive for a
 * (jet, receiver block) reads the SC slabs in chunk order -- a fixed order, whoever arrives last --, leaves the
 * total in slab 0 and runs the epilogue). */
typedef struct MpgEdgeFwd {
    const float* a; const float* c;       /* [B*N, 96], row stride ld_ac (0 = 96)             */
    int ld_ac;
    const float* mask;                    /* [B*N] (1 real / 0 padded) or NULL                */
    const void* W2img; const void* W3img; /* from mpg_pack_weights                            */
    const float* b2; const float* b3;     /* fe.net.1.bias [160], fe.net.2.bias [192]         */
    float* agg;                           /* [SC, B*N, 192]                                   */
    int B, N, SC;
    float alpha, agg_scale;
    const uint64_t* seed; uint32_t tag_base, thr; float dscale;  /* dropout: thr=round(256p), dscale=1/(1-p_eff) */
    int skip_masked;                      /* skip senders with mask == 0 (exact: they add 0)   */
    int f16;                              /* images and activations are fp16 hi/lo (else bf16)  */
    unsigned int* sign3;                  /* optional [B*RB*N][3][64] per-lane sign words of Z3 for the backward (NULL = off) */
    const unsigned int* nbr;              /* optional k-nearest-neighbour graph: [B*N][ceil(N/32)] words, bit j of row (b, i) set
                                             <=> sender j is a neighbour of receiver i (mpg_knn_sets); NULL = fully connected */
    void* stageE2;                        /* with sign3: E2 = fe.net.1's output (in the forward's operand scale) parked as fp16
                                             fragments [B*RB*N blocks][10][64 lanes][8] for mpg_edge_bwd / mpg_edge_dw */
    /* Edge features and row-tiled conditioning columns of MPLayer (mpgan/model.py:247-253, :297-313: delta_r, clabels,
     * mask_fne_np) -- MPG_EDGE_SCALARS scalars per edge, each times its own column of fe.net.0.weight:
     *   Z1(i, j) = a_i + c_j + sum_q es[b][j][q][i] * wq[q][:]
     * es is [B][N senders][MPG_EDGE_SCALARS][N receivers], wq [MPG_EDGE_SCALARS][96] (unused scalars: zero columns); NULL = none.
     * The scalars themselves (4 bytes per edge and scalar, not the 2F+ features per edge of the reference's edge matrix) are
     * the caller's: a norm of a coordinate difference, a gather from a [B] table. */
    const float* es; const float* wq;
    const int* order;                     /* optional [B]: workgroup g works on jet order[g] (mpg_jet_order); NULL = in index order */
    unsigned int* tickets;                /* mpg_edge_fwd_fn with SC > 1: [B*RB] arrival counters, ZERO on entry and left zero (the
                                             workgroup of a (jet, receiver block) that arrives last adds up the SC partial slabs);
                                             NULL = the epilogue form takes whole jets only (SC = 1) */
    int two_term;                         /* product form of the two dense layers: 0 = every product as three 16-bit terms (hi*hi +
                                             hi*lo + lo*hi: fp32-level pre-activations); 1 = fe.net.2 on TWO terms -- its input, the
                                             activation E2, rounded to the one fp16 value that is parked for the backward anyway,
                                             times W3 hi + lo: 2/9 fewer MFMAs, pre-activations of fe.net.2 known to ~1e-4 of their
                                             scale (an error that is independent from edge to edge and averages out in agg and in
                                             every gradient sum).  Other values, and 1 together with edge scalars: error -8. */
} MpgEdgeFwd;
#define MPG_EDGE_SCALARS 2
int mpg_edge_fwd(const MpgEdgeFwd* p, void* stream);

/* mpg_edge_fwd_fn: mpg_edge_fwd with the node network as the EPILOGUE of every workgroup -- one launch for
 *   A = fe(cat(x_i, x_j)) ; A * mask ; sum / mean ; x = fn(cat((A, x)))       (mpgan/model.py:256-279)
 * The workgroup that has aggregated a jet's 32 receivers runs the three layers of `fn` (the chain `c`, as mpg_chain takes
 * it) on them straight from LDS; agg reaches memory only as a by-product (p->agg, for fn.net.0's weight gradient; NULL =
 * not kept).  `c` is the chain mpg_chain would be given for the same call -- K1 = 192 columns of agg (c->A is not read:
 * the rows come from the kernel) followed by the node columns c->A2 [B*N, K - 192], three layers, outputs and dropout
 * sites as there -- and the results are bit-identical to mpg_edge_fwd followed by mpg_chain.
 * Covered: SC = 1, no edge scalars, fp16 images, layer widths K <= 224 -> N0, N1 in (224, 256] -> any N2 <= 256, no
 * gates / residuals / input dropout, one dropout mode for all sites.  Anything else returns MPG_FN_NA without
 * launching: the caller then runs the two launches.
 * `c2` (or NULL): one more mpg_chain call that runs behind fn on the same rows, in the same launch -- the NEXT MPLayer's
 * layer-1 node terms a | c = [W1a ; W1c] x + [b1 ; 0] of the rows fn has just produced (one layer, K = c's last N <= 32,
 * input c2->A = c->L[2].out), so that the next layer starts with its edge launch (mpgan/model.py:511-512: the loop over
 * mp_layers). */
#define MPG_FN_NA (-100)
int mpg_edge_fwd_fn(const MpgEdgeFwd* p, const MpgChain* c, const MpgChain* c2, void* stream);

/* mpg_knn_sets: the neighbour sets of MPLayer._getA_knn (mpgan/model.py:319-381) as bit masks for the fused edge kernels.
 * Per jet: d(i, j) = || s_j x_j - x_i + 1e-12 || over the F node features, s_j = (1 - 1e4) mask_j + 1e4 (:333-335: 1 for
 * a real sender, 1e4 for a zero-masked one); the senders of receiver i are those of rank [first, first + k) in ascending distance
 * (first = 0 with self loops, 1 without; equal distances in index order).  nbr is [B*N][ceil(N/32)] words.  Running
 * the fully-connected kernels over all N senders with these bits as a per-edge factor gives the reference's
 * gather / fe / sum over the k gathered neighbours (mean: agg_scale = 1/k); N <= 192. */
int mpg_knn_sets(const float* x, int ldx, const float* mask, int B, int N, int F, int k, int self_loops,
                 unsigned int* nbr, void* stream);

/* mpg_edge_bwd: autograd backward of the same span, data path.  Given dagg = dL/dagg and the
 * forward's sign words it produces
 *   da [SC, B*N, 96]  (partial over sender chunks),  dc [RB, B*N, 96]  (partial over receiver blocks of 32)
 * from stageE2 -- E2 = fe.net.1's output as mpg_edge_fwd parked it (required: its signs are phi'(Z2); nothing of the
 * forward is recomputed) -- and, when stageZ2 is non-NULL (weight gradients wanted), parks dZ2 = dL/d(fe.net.1's
 * pre-activation) as fp16 fragments [B*RB*N blocks][10][64 lanes][8] for mpg_edge_dw.  dZ2 is parked in units of
 * 2^-e of its (jet, receiver block) -- gradients have any magnitude, fp16 has 30 binades -- and gexp[b*RB + rb] = e
 * says which (e is chosen from max |dagg| of the block's receivers).
 * All images are fp16 (f16 must be 1, error -8): W3Timg / W2Timg the images of the transposed weights packed with the
 * forward's scales (dscale * 64, dscale * 16); W2img and b2 are not read.  The two gradient products run as two fp16
 * terms (image hi + lo times the gradient rounded to fp16 in a per-sender unit).  A sender chunk (ceil(N / SC) senders) may hold at most 160 senders (error -6: raise SC), and
 * the staging buffers must stay below 2 GiB (error -7). */
typedef struct MpgEdgeBwd {
    const float* a; const float* c; int ld_ac; const float* mask;
    const float* dagg; int ld_dagg;
    const unsigned int* sign3;            /* [B*RB*N][3][64] from mpg_edge_fwd                   */
    const void* W2img; const void* W3Timg; const void* W2Timg;
    const float* b2;
    float* da; float* dc;
    const void* stageE2;                  /* from mpg_edge_fwd (required)                        */
    void* stageZ2;                        /* optional output for mpg_edge_dw                     */
    int B, N, SC;
    float alpha, agg_scale;
    const uint64_t* seed; uint32_t tag_base, thr; float dscale;
    int f16;
    const unsigned int* nbr;              /* as MpgEdgeFwd.nbr */
    int* gexp;                            /* [B*RB] gradient-unit exponents of the parked dZ2 (required with stageE2/stageZ2) */
    const float* es; const float* wq;     /* as MpgEdgeFwd (NULL = none) */
    float* des;                           /* with es: dL/des, same layout (rows of skipped -- zero-masked -- senders are not written:
                                             clear it first) */
    float* daq;                           /* with es: [SC][B*N][MPG_EDGE_SCALARS][96] = sum_j es(i, j) * dZ1(i, j) per receiver;
                                             summed over its rows it is the gradient of wq */
    const int* order;                     /* as MpgEdgeFwd.order */
} MpgEdgeBwd;
int mpg_edge_bwd(const MpgEdgeBwd* p, void* stream);

/* mpg_edge_bwd_fn: mpg_edge_bwd with EPILOGUE chains on every workgroup's own jet -- one launch for the backward of an
 * MPLayer (mpgan/model.py:256-279) from dagg down to its input gradient, and on through the node network of the layer below:
 *   cdx  the "dx from da | dc" chain mpg_chain would be given behind this call: one layer, input A = p->da (96 columns) | A2 =
 *        p->dc, the stacked transposed W1 image, residual = the node path's dx, output dx [B*N, F <= 32];
 *   cnx  (or NULL) the node network's input-gradient chain of the NEXT-LOWER layer (three transposed layers with the gates of
 *        its forward, input = those dx rows with the trailing dropout's gate, outputs dz2, dz1, [dagg | dx]) as mpg_chain
 *        takes it.
 * A workgroup runs them on its 32 nodes when its own sender loop is done, while the fullest jets' workgroups are still in
 * theirs.  Results are bit-identical to mpg_edge_bwd followed by the mpg_chain calls.
 * Covered: a whole jet per workgroup (N <= 32, SC = 1), no edge scalars, bf16 images, one dropout mode; cnx widths K <= 32 ->
 * (224, 256] -> (224, 256] -> N <= 256.  Anything else returns MPG_FN_NA without launching. */
int mpg_edge_bwd_fn(const MpgEdgeBwd* p, const MpgChain* cdx, const MpgChain* cnx, void* stream);

/* mpg_edge_dw: weight gradients of fe.net.1 / fe.net.2 (and their biases) from the fragments parked by
 * mpg_edge_bwd:  dW3 = dscale * sum_e dZ3 E2^T [192,160], dW2 = dscale * sum_e dZ2 E1^T [160,96],
 * db3 = sum_e dZ3 [192], db2 = sum_e dZ2 [160]; E1 and dZ3 are rebuilt from a, c, dagg and the sign words.
 * ONE fp16 term per product: every operand a single fp16 value -- the parked ones as they were parked, the rebuilt ones rounded
 * once, in per-block dithered units so that the roundings are independent from edge to edge and average out over the ~1e5 edges a
 * weight gradient sums (csrc/edge_dw.hip) --, everything in ONE gradient unit 2^-min(gexp) for the launch.
 * `part` is scratch of nwg * 46,432 floats (per-workgroup partial sums); the nwg workgroups share the B*RB*N blocks
 * in runs of R consecutive senders (R = the largest divisor of N up to 6), and each may take at most 64 blocks, i.e.
 * R * ceil(B*RB*N / R / nwg) <= 64 (error -5 otherwise). */
typedef struct MpgEdgeDw {
    const float* a; const float* c; int ld_ac; const float* mask;
    const float* dagg; int ld_dagg;
    const unsigned int* sign3;
    const void* stageE2; const void* stageZ2;
    float* part; int nwg;
    float* dW3; float* dW2; float* db3; float* db2;
    int accumulate;                       /* add to dW3 / dW2 / db3 / db2 instead of overwriting */
    int B, N;
    float alpha, agg_scale;
    const uint64_t* seed; uint32_t tag_base, thr; float dscale;
    int f16;                              /* must be 1 */
    const unsigned int* nbr;              /* as MpgEdgeFwd.nbr */
    const int* gexp;                      /* [B*RB] from mpg_edge_bwd */
    const float* es; const float* wq;     /* as MpgEdgeFwd (NULL = none): E1 is rebuilt with them */
    int defer_reduce;                     /* 1: leave the per-workgroup partials in `part`; mpg_splitk_reduce_group_dw adds them up */
} MpgEdgeDw;
int mpg_edge_dw(const MpgEdgeDw* p, void* stream);
/* The reduction of an mpg_edge_dw launch that ran with defer_reduce = 1 AND the grouped split-K reduction of n (0 ... MPG_GROUP_MAX)
 * jobs of an earlier mpg_gemm_wgrad_group on the same stream, as ONE launch: the layer's edge-network and dense weight gradients
 * land in their buffers together, and the weight-gradient tail of a layer's backward is one dependent launch shorter.  Same sums
 * in the same order as mpg_edge_dw's own reduction + mpg_splitk_reduce_group. */
int mpg_splitk_reduce_group_dw(const MpgReduceJob* jobs, int n, const MpgEdgeDw* p, void* stream);

/* ---- the edge network on the k-nearest-neighbour graph's own rows ---------------------------------
 * mpg_knn_edge_fwd: replaces MPLayer._getA_knn's gather + self.fe(A) + mask multiply + sum/mean for fully_connected=False
 * (mpgan/model.py:319-381, :256-267) on the B*N*k edge ROWS the reference builds there -- not on all N*N pairs with the neighbour
 * bit as a factor, as mpg_edge_fwd does with MpgEdgeFwd.nbr.  Row (b, i, r), global index (b N + i) k + r, pairs receiver i with
 * the r-th set bit (ascending sender index) of nbr[(b N + i) ceil(N/32) ..] as mpg_knn_sets writes them:
 *   agg[b,i,:] = agg_scale * sum_{r < k} mask[b, j(i, r)] * fe([x_i ; x_j(i, r)])     (rows added in ascending r, no atomics)
 * a, c, the W2 / W3 images, biases, scales, product form (three fp16 terms) and dropout draws (keyed by the DENSE edge row
 * (b N + i) N + j) are those of mpg_edge_fwd: a dense and a sparse launch of one call keep the same elements.
 * A workgroup takes RW consecutive receivers of a jet (RW * k rows in tiles of 32; RW * k * 784 bytes of LDS <= 160 KiB, error -6).
 * With E1 != NULL it parks, row-major and in fp32, what the backward and the weight-gradient GEMMs read: E1 [B*N*k, 96] and
 * E2 [B*N*k, 160] = the inputs of fe.net.1 / fe.net.2 as the reference has them (dropout scale included; rows of zero-masked
 * senders are zero), and sign3 [B*N*k][6][2] 16-bit words: bit 4g + t of word (tile m, lane half h) set <=> Z3[32m + 8g + 4h + t] <= 0.
 * N <= 192 (mpg_knn_sets), 0 < k <= N. */
typedef struct MpgKnnEdgeFwd {
    const float* a; const float* c; int ld_ac;   /* as MpgEdgeFwd                                    */
    const float* mask;                           /* [B*N] or NULL                                    */
    const unsigned int* nbr;                     /* [B*N][ceil(N/32)] from mpg_knn_sets (required)   */
    const void* W2img; const void* W3img;        /* the fp16 images of MpgEdgeFwd                    */
    const float* b2; const float* b3;
    float* agg;                                  /* [B*N, 192]                                       */
    int B, N, k, RW;
    float alpha, agg_scale;
    const uint64_t* seed; uint32_t tag_base, thr; float dscale;
    float* E1; float* E2; unsigned short* sign3; /* parked for the backward: all three or none       */
} MpgKnnEdgeFwd;
int mpg_knn_edge_fwd(const MpgKnnEdgeFwd* p, void* stream);

/* mpg_knn_edge_bwd: autograd backward of the same span (the backward of mpgan/model.py:256-267 and of the gather of :319-381),
 * data path, from dagg and what mpg_knn_edge_fwd parked.  Per row: dZ3, dZ2 = W3^T dZ3, dZ1 = W2^T dZ2 through the parked gates
 * and the regenerated dropout keeps (W3Timg / W2Timg as MpgEdgeBwd's; three fp16 terms, the gradient split hi + lo in a
 * power-of-two unit per row).  dZ1 [B*N*k, 96] is always written (scratch of the launch), dZ2 [B*N*k, 160] and dZ3 [B*N*k, 192]
 * when non-NULL (both or none): with E1 / E2 they are the operands of the weight-gradient GEMMs of fe.net.1 / fe.net.2; rows
 * of zero-masked senders are zero.  A second kernel of the same call then writes dadc [B*N, 192] = da | dc:
 *   da[b,i,:] = sum_{r < k} dZ1(b, i, r)  in ascending r;   dc[b,j,:] = sum over the receivers i that list j, in ascending i
 * (it walks column j of the bit words) -- fixed orders, no atomics. */
typedef struct MpgKnnEdgeBwd {
    const float* mask; const unsigned int* nbr;
    const void* W3Timg; const void* W2Timg;
    const float* dagg; int ld_dagg;              /* [B*N, >= 192], row stride ld_dagg                */
    int B, N, k, RW;
    float alpha, agg_scale;
    const uint64_t* seed; uint32_t tag_base, thr; float dscale;
    const float* E1; const float* E2; const unsigned short* sign3;   /* from mpg_knn_edge_fwd       */
    float* dZ1; float* dZ2; float* dZ3;
    float* dadc;
} MpgKnnEdgeBwd;
int mpg_knn_edge_bwd(const MpgKnnEdgeBwd* p, void* stream);

/* mpg_knn_edge_jvp: the second-order half of the same span -- what a twice-differentiable edge aggregation (the gradient penalty,
 * train.py:286-324) needs beside mpg_knn_edge_fwd / _bwd -- on the same rows, tiles and parked gates (E1 / E2 > 0 where kept,
 * sign3, the regenerated keep words).  Two modes:
 *   dot (ta == NULL)   E3_row = gate3 (W3 E2_row + b3) from the parked E2;  rowdot[row] = <E3_row, dagg_i>;
 *                      dmask[b,j] = agg_scale * sum of rowdot over the rows that list sender j, in ascending receiver order:
 *                      the gradient of sum_i <agg_i, dagg_i> with respect to mask_j.
 *   jvp (ta != NULL)   T1 = gate1 (ta_i + tc_j), T2 = gate2 W2 T1, T3 = gate3 W3 T2 (tangent rows split hi + lo in fp16 in a
 *                      power-of-two unit of their own row, three terms);  T1 [B*N*k, 96] and T2 [B*N*k, 160] leave row-major in
 *                      fp32 (dropout scale included) when non-NULL;  aggt[b,i,:] = agg_scale * sum_r (mask_j T3 + mu_j E3) in
 *                      ascending r when non-NULL (mu NULL: no E3 term);  rowdot[row] = <T3_row, dagg_i> and dmask as above
 *                      when non-NULL (both or none).
 * A row takes part when mask_j != 0 or mu_j != 0; a tile without such a row is skipped, its rows written as zeros.
 * Errors as mpg_knn_edge_fwd: -1 sizes, -2 a required pointer is NULL, -3 E1 / E2 / sign3 (or rowdot / dmask, or ta / tc) not
 * all-or-none, -4 alpha outside [0, 1], -5 a row stride below its width or not a multiple of 4, -6 RW * k * 784 bytes of LDS
 * above 160 KiB, -7 B * N * N beyond the 32-bit dropout key.  No atomics; nothing depends on which wave finishes first. */
typedef struct MpgKnnEdgeJvp {
    const unsigned int* nbr; const float* mask; const float* mu;   /* mask, mu: [B*N] or NULL                        */
    const float* dagg; int ld_dagg;                                 /* [B*N, >= 192]                                  */
    const float* ta; const float* tc; int ld_t;                     /* [B*N, >= 96] each: u W1a^T, u W1b^T (no bias)  */
    const void* W2img; const void* W3img; const float* b3;          /* as MpgKnnEdgeFwd                               */
    const float* E1; const float* E2; const unsigned short* sign3;  /* from mpg_knn_edge_fwd                          */
    float* T1; float* T2; float* aggt; float* rowdot; float* dmask;
    int B, N, k, RW;
    float alpha, agg_scale;
    const uint64_t* seed; uint32_t tag_base, thr; float dscale;
} MpgKnnEdgeJvp;
int mpg_knn_edge_jvp(const MpgKnnEdgeJvp* p, void* stream);

/* ---- attention core of GAPT's MAB ---------------------------------------------------------------
 * mpg_attn_fwd / mpg_attn_bwd: per (jet b, head h), d = E / H:
 *     P = softmax_s( q_h k_h^T / sqrt(d)  with keys s where ignore[b,s] != 0 at -inf ),   o_h = P v_h
 * i.e. what nn.MultiheadAttention does between its in- and out-projection as called by MAB.forward
 * (gapt/model.py:127-129).  q [B*L, ldq], k/v [B*S, ldk/ldv], o [B*L, ldo] hold the H heads side by
 * side (head h = columns h*d .. h*d+d-1); P (B*H*L*S floats, layout private to the pair of kernels) is written by fwd and read by bwd;
 * ignore [B*S] floats (1 = padded key) or NULL.  bwd takes d_o = dL/do and writes dq, dk, dv.
 * A query whose keys are all ignored gets zero attention weights (torch's _safe_softmax meaning); all outputs and gradients
 * stay finite. */
typedef struct MpgAttn {
    const float* q; const float* k; const float* v; int ldq, ldk, ldv;
    const float* ignore;
    float* o; int ldo;
    float* P;
    const float* d_o;
    float* dq; float* dk; float* dv; int lddq, lddk, lddv;
    int B, L, S, H, d;
} MpgAttn;
int mpg_attn_fwd(const MpgAttn* p, void* stream);
int mpg_attn_bwd(const MpgAttn* p, void* stream);

/* mpg_attn_dd: the second-order half -- what a twice-differentiable attention core (the gradient penalty through GAPT's MAB) needs
 * beyond the two calls above.  With dq, dk, dv = mpg_attn_bwd(q, k, v, d_o) and cotangents uq, uk, uv on them, it writes the
 * gradients of  Phi = <uq, dq> + <uk, dk> + <uv, dv>  with respect to q, k, v and d_o (c = 1 / sqrt(d), rowsum over keys):
 *     A = d_o v^T,  a = rowsum(P*A),  dS = P*(A - a);    Sd = c (uq k^T + q uk^T),  r = rowsum(P*Sd),  Pd = P*(Sd - r)
 *     M = Sd*(A - a) - r*A + d_o uv^T,   D2 = P*(M - rowsum(P*M))
 *     gq = c (D2 k + dS uk)    gk = c (D2^T q + dS^T uq)    gv = Pd^T d_o    gdo = Pd v + P uv
 * Operands as in MpgAttn (heads side by side, any row stride >= H * d, unit column stride); P as mpg_attn_fwd wrote it for the same
 * B, L, S, H, d (the layout is taken from the predicate the other two entry points use).  uq / uk / uv may be NULL (= zero) and any
 * output may be NULL (= not wanted): the work behind them is skipped, not only the store.  Ignored keys contribute exactly zero, a
 * jet without a real key gets exact zeros in all four outputs.  Covers d in {8, 16, 32} and 1 <= L, S <= 160; no L x S tile is
 * written anywhere; every sum runs in a fixed order (no atomics: two launches give the same bits).
 * Errors, before anything is launched: -1 sizes outside the above, -2 q / k / v / d_o / P is NULL, -5 a row stride below H * d. */
typedef struct MpgAttnDD {
    const float* q; const float* k; const float* v; const float* d_o; int ldq, ldk, ldv, ldo;
    const float* uq; const float* uk; const float* uv; int lduq, lduk, lduv;
    const float* ignore;
    const float* P;
    float* gq; float* gk; float* gv; float* gdo; int ldgq, ldgk, ldgv, ldgdo;
    int B, L, S, H, d;
} MpgAttnDD;
int mpg_attn_dd(const MpgAttnDD* p, void* stream);

/* ---- the per-jet pieces around the message-passing layers ----------------------------------------
 * mpg_rank_mask: MPGenerator._get_mask, mask_c branch (mpgan/model.py:689-699; GAPT_G :255-258): with
 * n_b = int(labels[b] * N), mask[b, i] = 1 for the n_b particles of jet b with the smallest first feature
 * x[b*ld_jet + i*ld_part] (rank = argsort(argsort(.)); ties by index), else 0.  mask is [B, N] contiguous; `ignore`
 * (or NULL) receives 1 - mask in the same pass: the key mask GAPT's attention blocks take (_attn_mask, gapt/model.py:194-202). */
int mpg_rank_mask(const float* x, int ld_jet, int ld_part, const float* labels, int ld_lab, int B, int N,
                  float* mask, float* ignore, void* stream);

/* mpg_jet_order: the jets of a batch by decreasing number of unmasked particles (ties by index), order[0] the fullest --
 * MpgEdgeFwd.order / MpgEdgeBwd.order.  The edge kernels take a workgroup per jet and as long as the jet has senders; when a
 * launch has more workgroups than the chip has CUs (the discriminator's real + generated batch), handing them out heaviest
 * first is the classic longest-processing-time rule: 136 -> 113 us for 512 gluon-like jets.  No effect on any result.
 * B + N + 2 + ceil(B / 64) * (N + 1) <= 16384 (error -2). */
int mpg_jet_order(const float* mask, int B, int N, int* order, void* stream);

/* mpg_gen_tail_fwd / _bwd: MPNet._final_activation (:533-538) + MPGenerator._final_mask (:741-757) on V = B*N rows:
 * out[v, 0:F] = act(y[v, 0:F]) (act 0 none, 1 tanh, 2 sigmoid), out[v, F] = mask[v] - 0.5 when mask != NULL;
 * backward dy = dout[:, 0:F] * act'(out).  Row strides ldy / ldo / ldd let the output land inside a larger batch. */
int mpg_gen_tail_fwd(const float* y, int ldy, const float* mask, float* out, int ldo, int V, int F, int act, void* stream);
int mpg_gen_tail_bwd(const float* dout, int ldd, const float* out, int ldo, float* dy, int ldy, int V, int F, int act,
                     void* stream);

/* mpg_disc_head_fwd / _bwd: MPDiscriminator._post_mp (masked sum or mean over the particles, :812-829), fnd_layer =
 * one Linear(F -> 1) followed by Dropout (LinearNet, :77-83) and the final sigmoid (:537); also GAPT_D's
 * final_fc + sigmoid (gapt/model.py:344) with N = 1.
 *   fwd:  out[b] = act( keep_b * ( pool_b( sum_i mask[b,i] y[b,i,:] ) . w + bias ) )
 *   bwd:  dy[b,i,f], and dw / db of the Linear (added to when accumulate), from
 *         loss < 0 : gout[b] = dL/dout[b] handed in by autograd
 *         loss >= 0: the loss named (0 ls, 1 og, 2 w, 3 hinge: calc_D_loss / calc_G_loss, train.py:331-395, :465-476),
 *                    jets [0, n_real) scored as real and the rest as generated (gen_step: all as real, generator
 *                    form), each term times inv_count; loss_out receives the sum of the terms.  With targets != NULL jet b
 *                    is scored against targets[b] (any value: the ls / og terms and gradients with t = targets[b]; w / hinge
 *                    take t > 0.5 as "real"), and *loss_extra, when given, is added to loss_out: the two outputs of
 *                    mpg_label_targets.  Both NULL: the results of the 1 / 0 form, bit for bit.
 * aux [2B] and pooled [B,F] are scratch written by fwd and read by bwd. */
typedef struct MpgDiscHead {
    const float* y; int ldy;              /* [B, N, F], row (particle) stride ldy                  */
    const float* mask;                    /* [B, N] or NULL                                        */
    const float* w; const float* bias;    /* Linear(F -> 1): weight [F], bias [1] or NULL          */
    int B, N, F;
    int mean;                             /* pooling: 0 sum, 1 mean (mask sum + 1e-12, or N)       */
    int sigmoid;
    const uint64_t* seed; uint32_t tag, thr; float dscale;   /* dropout on the Linear's output     */
    float* out;                           /* [B]                                                   */
    float* pooled; float* aux;
    int loss, gen_step, n_real; float inv_count;
    const float* gout;
    float* terms; float* loss_out;        /* [B] scratch; scalar                                   */
    float* dy; int ld_dy;                 /* [B, N, F] or NULL                                     */
    float* dw; float* db; int accumulate;
    const float* targets;                 /* [B] or NULL: jet b is scored against targets[b] instead of 1 / 0 (loss >= 0) */
    const float* loss_extra;              /* scalar or NULL: added to the sum of the terms in loss_out                    */
} MpgDiscHead;
int mpg_disc_head_fwd(const MpgDiscHead* p, void* stream);
int mpg_disc_head_bwd(const MpgDiscHead* p, void* stream);
/* mpg_disc_head_loss: forward, the named loss and the whole backward of the head in one pass -- p->loss >= 0 with its
 * fields set as for mpg_disc_head_bwd: a jet's loss gradient needs nothing but its own output, so the wave that has pooled
 * a jet goes straight on to dy (one launch + the small reduction for the loss value and dw / db, instead of mpg_disc_head_fwd
 * + mpg_disc_head_bwd).  Same results as the two calls. */
int mpg_disc_head_loss(const MpgDiscHead* p, void* stream);

/* mpg_disc_head_dd: what a twice-differentiable head (the gradient penalty through MPDiscriminator / GAPT_D) needs beside
 * mpg_disc_head_fwd.  There the mask is real-valued and takes a gradient, which mpg_disc_head_bwd does not form.  Per jet, with
 * d = 1 (sum), sum_i m_i + 1e-12 (mean, mask) or N (mean, no mask), kappa the keep-and-scale of the output dropout (regenerated
 * from seed / tag / thr as the forward draws it), phi the sigmoid or the identity:
 *     t_i = <w, y_i>,  S = sum_i m_i t_i,  s = S / d + b,  z = kappa s,  out = phi(z),  c = S / d (mean with mask) or 0
 * mode 0, the first derivative for the cotangent g on out (g NULL = zero):  gh = g phi'(z) kappa
 *     gy_i = gh m_i w / d      gm_i = gh (t_i - c) / d      gw = sum_b gh sum_i m_i y_i / d      gb = sum_b gh
 * mode 1, the second derivative: with cotangents U_i on gy_i and mu_i on gm_i (either may be NULL = zero) and
 *     Phi = sum_i <U_i, gy_i> + sum_i mu_i gm_i = gh R,   a_i = <w, U_i>,  Q = sum_i mu_i (mean with mask; 0 otherwise),
 *     R = (sum_i m_i a_i + sum_i mu_i t_i - c Q) / d,     H = g kappa^2 phi''(z) R,     e_i = (mu_i - Q m_i / d) / d
 * it writes the gradients of Phi:
 *     gg = kappa phi'(z) R                          (with respect to g)
 *     gy_i = (H m_i / d + gh e_i) w
 *     gm_i = H (t_i - c) / d + gh ((a_i - Q (t_i - c) / d) / d - [mean with mask] R / d)
 *     gw = sum_b ( sum_i (H m_i / d + gh e_i) y_i + (gh / d) sum_i m_i U_i )        gb = sum_b H
 * Under the mean with a mask the differences t_i - c, a_i d - sum_j m_j a_j and mu_i d - Q m_i are formed as single sums of pairwise
 * terms (sum_j m_j (t_i - t_j) + 1e-12 t_i, ...): a jet with one real particle, where they are 1e-12 of their terms, keeps its digits.
 * One wave per jet, fp32; every sum over a jet's particles and over the features runs in index order, gw / gb across jets through
 * per-jet rows `part` [B, F + 1] and a fixed-order reduction; no atomics: two launches give the same bits.  Any output may be NULL
 * (= not wanted; `part` is needed for gw / gb) and the work behind it is skipped, as is the work behind a NULL U / mu.
 * mask NULL: m_i = 1, gm must be NULL.  1 <= N <= 1024.
 * Errors, before anything is launched: -1 sizes or mode, -2 a required pointer is NULL, -5 a row stride below F. */
typedef struct MpgDiscHeadDD {
    const float* y; int ldy;              /* [B, N, F], row (particle) stride ldy                  */
    const float* mask;                    /* [B, N] or NULL                                        */
    const float* w; const float* bias;    /* weight [F], bias [1] or NULL                          */
    int B, N, F, mean, sigmoid;
    const uint64_t* seed; uint32_t tag, thr; float dscale;
    int mode;
    const float* g;                       /* [B]: the cotangent on out                             */
    const float* U; int ldu;              /* [B, N, F] or NULL (mode 1)                            */
    const float* mu;                      /* [B, N] or NULL (mode 1)                               */
    float* gy; int ld_gy;                 /* [B, N, F] or NULL                                     */
    float* gm;                            /* [B, N] or NULL                                        */
    float* gg;                            /* [B] or NULL (mode 1)                                  */
    float* part;                          /* [B, F + 1] scratch for gw / gb                        */
    float* gw; float* gb;                 /* [F], [1] or NULL                                      */
} MpgDiscHeadDD;
int mpg_disc_head_dd(const MpgDiscHeadDD* p, void* stream);

/* mpg_bridge_fwd / mpg_bridge_bwd: the rows between a GAPT generator's last attention block and the discriminator's first
 * one as ONE launch each way (csrc/bridge.hip) -- gen's final_fc (gapt/model.py:248, :263: Linear K -> F, no activation) and
 * final tanh (:265), then disc's input_embedding (:300-302, :336-339: Linear F -> E, LeakyReLU, dropout), which otherwise run
 * as mpg_gemm + mpg_gen_tail_fwd + mpg_gemm (and mpg_gate + mpg_gemm + mpg_gen_tail_bwd + mpg_gemm on the way back):
 *   rows >= row0 (generated):  feat = act1(W1 x + b1), written to feat ;  rows < row0 (real jets): feat is read
 *   every row:                 e = dropout(lrelu(W2 feat + b2))          (e == NULL: stage 1 alone)
 * x [M - row0, K], feat [M, F], e [M, E]; K = E = 64, F in 1..4 or 8; act1: mpg_gen_tail_fwd's codes.
 * bwd: g2 = ge through stage 2's dropout and LeakyReLU (what mpg_gate gives: the operand of W2's weight gradient), all rows;
 * for rows >= row0, when g1 or dx is given: g1 = (g2 W2 + gfeat) act1'(feat) (the operand of W1's weight gradient) and
 * dx = g1 W1.  Any of g2, g1, dx, gfeat may be NULL. */
typedef struct MpgBridge {
    const float* x; int ldx;
    const float* W1; const float* b1;       /* [F, K], [F] or NULL                                   */
    int act1;
    float* feat; int ldf;
    int M, row0, K, F, E;
    const float* W2; const float* b2;       /* [E, F], [E] or NULL                                   */
    int act2; float alpha;
    const uint64_t* seed; uint32_t tag, thr; float dscale;   /* dropout on e (site tag)              */
    float* e; int lde;
} MpgBridge;
typedef struct MpgBridgeBwd {
    const float* ge; int ldge;              /* [M, E] gradient with respect to e                     */
    const float* e; int lde;                /* stage 2's saved output                                */
    const float* feat; int ldf;
    const float* gfeat; int ldgf;           /* [M - row0, F] further gradient into feat, or NULL     */
    const float* W1; const float* W2;
    int M, row0, K, F, E, act1, act2; float alpha;
    const uint64_t* seed; uint32_t tag, thr; float dscale;
    float* g2; int ldg2;                    /* [M, E]                                                */
    float* g1; int ldg1;                    /* [M - row0, F]                                         */
    float* dx; int lddx;                    /* [M - row0, K]                                         */
} MpgBridgeBwd;
int mpg_bridge_fwd(const MpgBridge* p, void* stream);
int mpg_bridge_bwd(const MpgBridgeBwd* p, void* stream);

/* mpg_mab_fwd / mpg_mab_bwd: one launch per MAB.forward (gapt/model.py:124-139) and one for its backward, for sets of at
 * most 160 tokens (L, S <= 32: a wave or two per jet; 33 ... 160 -- --num-hits 150, setup_training.py:415 --: a workgroup per
 * jet, a wave per tile of 32 tokens, key tiles walked with a running maximum / sum, projections made once per tile and
 * shared through LDS), E in {32, 64}, heads of 16 features, with or without the
 * two layer norms (csrc/mab_fwd.hip, mab_bwd.hip, mab_bwds.hip over mab_common.h; anything else runs block by block through mpg_gemm / mpg_attn_* / mpg_gate):
 *   q = x Wq' + bq, k|v = y Wkv' + bkv ; o = softmax(q k' / 4 + key mask) v per head ; za = x + o Wo' + bo ;
 *   z = dropout(za, site tag) ; u = z Wf' + bf ; out = dropout(z + dropout(act(u), site tag+1), site tag+2)
 * x [B*L, E] queries, y [B*S, E] keys/values (y == x: self-attention), ignore [B*S] floats (1 = padded key) or NULL.
 * Win / Wo / Wf: fp16 hi|lo images (mpg_pack_weights, scale wscale) of in_proj_weight [3E, E], out_proj.weight and
 * ff.net.0.weight [E, E]; activations are split as ascale * value.  fwd writes out and, when given, save_o (attention
 * output before the out-projection) and save_z [B*L, E] -- the two activations the weight gradients and the backward need.
 * bwd recomputes q, k, v, P and u from x, y and save_z, and writes the input gradients dx (dy when y != x) and the three
 * pre-activation gradients whose products with (x | y, save_o, save_z) are the weight gradients:
 *   dq [B*L, :E] / dk, dv [B*S] (row strides lddq / lddkv), dza, du [B*L, E].
 * WinT / WoT / WfT: bf16 images of the transposed weights ([E, 3E], [E, E], [E, E], scale 1).
 * A query whose keys are all ignored gets zero attention weights (o = 0, za = x + bo) on every kernel behind these entry
 * points, mpg_mab_chain_fwd included; all outputs and gradients stay finite (tests/test_gpu_mab_masks.py). */
typedef struct MpgMab {
    const float* x; int ldx;
    const float* y; int ldy;
    const float* ignore;
    const void* Win; const float* bin;
    const void* Wo; const float* bo;
    const void* Wf; const float* bf;
    int B, L, S, E, H;
    float alpha; int ff_act;
    const uint64_t* seed; uint32_t tag; uint32_t thr_mab; float sc_mab; uint32_t thr_ff; float sc_ff;
    float wscale, ascale;
    float* out; int ldo;
    float* save_o; float* save_z;
    const void* WinT; const void* WoT; const void* WfT;
    const float* dout; int lddout;
    float* dx; int lddx; float* dy; int lddy;
    float* dq; int lddq; float* dk; float* dv; int lddkv;
    float* dza; float* du;
    /* layer_norm=True (gapt/model.py:118-120, :131-136): nn.LayerNorm(E) behind each residual, or all NULL.  za -> norm1 -> dropout;
     * z + ff(z) -> norm2 -> dropout.  fwd keeps za (before norm1) in save_za for the backward; bwd writes, per row, the
     * gradient with respect to each norm's OUTPUT (dn1, dn2: their column sums are the norms' bias gradients) and that times
     * the normalised input (gn1, gn2: column sums = weight gradients).  One wave per jet (the two-wave kernels step aside). */
    const float* ln1_w; const float* ln1_b; const float* ln2_w; const float* ln2_b; float ln_eps;
    float* save_za;
    float* dn1; float* gn1; float* dn2; float* gn2;
} MpgMab;
int mpg_mab_fwd(const MpgMab* p, void* stream);
int mpg_mab_bwd(const MpgMab* p, void* stream);
/* mpg_mab_chain_fwd: up to MPG_MAB_CHAIN_MAX self-attention blocks applied one after the other -- the loop over the SABs of
 * GAPT_G / GAPT_D (gapt/model.py:261-262, :341-342) -- in ONE launch: blk[b] is the argument block mpg_mab_fwd would be given
 * for block b (y == x; blk[b].x == blk[b-1].out; one shape, one key mask).  A wave keeps its jet's rows in registers from
 * block to block; each block still writes its out / save_o / save_z.  Same results as the n single launches. */
#define MPG_MAB_CHAIN_MAX 4
typedef struct MpgMabChain { MpgMab blk[MPG_MAB_CHAIN_MAX]; int n; } MpgMabChain;
int mpg_mab_chain_fwd(const MpgMabChain* c, void* stream);

/* mpg_layernorm_fwd / _bwd: nn.LayerNorm(E) over the rows of x [M, E] -- MAB.norm1 / norm2 of GAPT with layer_norm
 * (gapt/model.py:118-120, :131-136).  fwd writes y and stats [M][mean, rstd]; bwd writes dx and, through `part`
 * (scratch of nwaves * 2 * E floats, nwaves a multiple of 4 = waves of the launch), dw = sum_rows g * xhat and
 * db = sum_rows g in a fixed summation order (added to when accumulate). */
int mpg_layernorm_fwd(const float* x, int ldx, const float* w, const float* b, float* y, int ldy, float* stats, int M,
                      int E, float eps, void* stream);
int mpg_layernorm_bwd(const float* g, int ldg, const float* x, int ldx, const float* w, const float* stats, float* dx,
                      int lddx, float* part, int nwaves, float* dw, float* db, int accumulate, int M, int E, void* stream);

/* mpg_batchnorm_*: nn.BatchNorm1d(F) over the rows of x [M, F] -- LinearNet's optional normalisation behind each
 * LeakyReLU (mpgan/model.py:58-60, :80-81).  stats writes the batch mean and BIASED variance (two passes; `part` is scratch
 * of nchunk * F floats); apply normalises with whatever mean / var it is given (batch statistics in training, running
 * statistics in eval) and the affine w, b (NULL = 1, 0); bwd (training statistics) writes dx and dw = sum g xhat,
 * db = sum g (added to when accumulate) with `part` of 2 * nchunk * F and `sums` of 2 * F floats as scratch. */
int mpg_batchnorm_stats(const float* x, int ldx, int M, int F, float* part, int nchunk, float* mean, float* var, void* stream);
int mpg_batchnorm_apply(const float* x, int ldx, const float* mean, const float* var, const float* w, const float* b, float eps,
                        float* y, int ldy, int M, int F, void* stream);
int mpg_batchnorm_bwd(const float* g, int ldg, const float* x, int ldx, const float* mean, const float* var, const float* w, float eps,
                      float* part, int nchunk, float* sums, float* dx, int lddx, float* dw, float* db, int accumulate, int M, int F,
                      void* stream);

/* ---- optimisers --------------------------------------------------------------------------------
 * One launch over one flat buffer of n parameters; `gscale` multiplies the gradient first (1/world after a
 * summing all-reduce).  They replace torch.optim.*.step() as the reference builds them (setup_training.py:1511-1523):
 * mpg_rmsprop  (--optimizer rmsprop, the default): v = alpha v + (1-alpha) g^2; p -= lr g / (sqrt(v) + eps)
 * mpg_adam     (--optimizer adam; weight_decay 5e-4 there): torch.optim.Adam with L2 weight decay; `step` is a
 *              device float holding the number of steps taken so far (advanced by the call)
 * mpg_adadelta (--optimizer adadelta): torch.optim.Adadelta (rho 0.9, eps 1e-6 by default).
 * zero_grad != 0: g is cleared behind its last use -- optimizer.zero_grad() of the NEXT train_D / train_G (train.py:419,
 * :494) without a launch of its own.
 * counter != NULL: *counter += counter_add by the same launch -- the device-resident dropout / noise seed moved on to the
 * next iteration's value by the iteration's last launch (no kernel may be reading it on another stream); NULL: nothing. */
int mpg_rmsprop(float* p, float* g, float* v, uint64_t n, float lr, float alpha, float eps, float gscale, int zero_grad,
                uint64_t* counter, uint64_t counter_add, void* stream);
int mpg_adam(float* p, float* g, float* m, float* v, float* step, uint64_t n, float lr, float beta1,
             float beta2, float eps, float weight_decay, float gscale, int zero_grad, uint64_t* counter, uint64_t counter_add,
             void* stream);
int mpg_adadelta(float* p, float* g, float* v, float* u, uint64_t n, float lr, float rho, float eps,
                 float gscale, int zero_grad, uint64_t* counter, uint64_t counter_add, void* stream);

/* The averaged forms: the same launch also folds the new parameters into an exponential moving average e [n] of them (Yazici
 * et al. 2019; the G_ema of StyleGAN2-ADA).  The reference has no such option (its answer to an oscillating generator is
 * G_best_epoch.pt, train.py:794-797): this statement is the specification.
 * state: uint32[2] = {t, ticket} in device memory -- t counts the averaged launches made so far; the ticket is the launch's
 * arrival counter and reads 0 between launches.  For every element i, with p_new the value the optimiser stores in p[i] and t
 * the step word as it stood before the launch:
 *   if t < start:   e[i] = p_new                                        (the average follows the weights until averaging begins)
 *   else:
 *       k      = (float) min(t - start, 2^24)                           (exact)
 *       beta_t = warmup ? min(beta, (1 + k) / (10 + k)) : beta           (two fp32 sums, ONE fp32 division)
 *       om     = 1 - beta_t                                             (ONE fp32 subtraction)
 *       d = p_new - e[i];  m = om * d;  e[i] = e[i] + m                 (THREE fp32 operations)
 * Every operation rounds to nearest even on its own; nothing is contracted into a fused multiply-add.  p, the optimiser's
 * moments, g and *counter come out bit for bit as from the entry point without the average.
 * Every workgroup reads t before anything else and arrives on the ticket last; the one that arrives last writes t + 1 and puts
 * the ticket back to 0: exactly one write per launch, behind every read of the old value, and no launch of its own.
 * A NULL block, ema or state, beta outside [0, 1) or a NaN, start < 0, n == 0: -1.
 * mpg_ema_update_host: the rule alone, compiled from the same body for the host, on host memory: e[i] <- rule(e[i], p_new[i])
 * for i < n at step word t.  No HIP call; the same refusals. */
typedef struct MpgEma {
    float* ema;
    uint32_t* state;   /* t, ticket */
    float beta;
    int start;
    int warmup;
} MpgEma;
int mpg_rmsprop_ema(float* p, float* g, float* v, uint64_t n, float lr, float alpha, float eps, float gscale, int zero_grad,
                    uint64_t* counter, uint64_t counter_add, const MpgEma* ema, void* stream);
int mpg_adam_ema(float* p, float* g, float* m, float* v, float* step, uint64_t n, float lr, float beta1,
                 float beta2, float eps, float weight_decay, float gscale, int zero_grad, uint64_t* counter, uint64_t counter_add,
                 const MpgEma* ema, void* stream);
int mpg_adadelta_ema(float* p, float* g, float* v, float* u, uint64_t n, float lr, float rho, float eps,
                     float gscale, int zero_grad, uint64_t* counter, uint64_t counter_add, const MpgEma* ema, void* stream);
int mpg_ema_update_host(float* e, const float* p_new, uint64_t n, uint32_t t, float beta, int start, int warmup);

/* The optimizer-step control: a learning-rate schedule and gradient clipping by the global L2 norm (torch.nn.utils.
 * clip_grad_norm_) for one network, as ONE launch in front of its optimizer launch -- inside a captured hipGraph, where lr and
 * gscale passed by value would be constants.  The reference has neither option: this statement is the specification.
 * Device state: state uint32[2] = {t, ticket} -- t counts the controlled steps this optimizer has taken, the ticket is the launch's
 * arrival counter and reads 0 between launches; base float[1], the base learning rate; out float[4] = {lr_eff, s, norm, factor}.
 * mpg_step_control computes, for the step about to be taken, with t as it stood before the launch:
 *   factor: nknots == 0: 1.  Otherwise over the knots (knot_step[k], knot_f[k]), k < nknots <= MPG_LR_KNOTS, steps strictly
 *           increasing and <= 2^24, factors finite and >= 0:
 *             t <= knot_step[0]: knot_f[0];  t >= knot_step[last]: knot_f[last];  else on the segment knot_step[k] <= t < knot_step[k+1]:
 *             w = (float)(t - knot_step[k]) / (float)(knot_step[k+1] - knot_step[k])       (both conversions exact, ONE fp32 division)
 *             factor = knot_f[k] + w * (knot_f[k+1] - knot_f[k])                            (THREE fp32 operations)
 *   lr_eff = base * factor
 *   norm   = (float) sqrt(sum_i ((double)(gscale * g[i]))^2) over the n gradients: the product in fp32, squares and sums in fp64
 *            in a fixed order that depends on n alone -- min(256, ceil(n / 256)) workgroups of 256 threads, every thread its strided
 *            elements in index order, every workgroup a fixed tree, the workgroup that arrives last on the ticket the partials in
 *            workgroup order: two launches on one buffer give the same bits.  Computed when max_norm clips or want_norm != 0;
 *            otherwise 0 is written, the launch is one workgroup and reads no gradient.
 *   gmul   = max_norm clips ? min(1, max_norm / (norm + 1e-6f)) : 1      (max_norm <= 0 or +inf: no clipping; a NaN quotient stays)
 *   s      = gscale * gmul
 * then t <- t + 1 (stopping at 2^32 - 1) and ticket <- 0, by the workgroup that arrived last.  Every fp32 operation rounds to
 * nearest even on its own; nothing is contracted.  Non-finite gradients get no special treatment.
 * partials: 256 doubles of scratch in device memory, the caller's, allocated once.
 * A NULL block, state, base, out or partials; nknots outside [0, MPG_LR_KNOTS]; knot steps unordered or above 2^24; a factor
 * negative or not finite; a NaN max_norm or gscale; a norm to compute with g NULL or n == 0: -1.
 * mpg_step_control_host: the same rule from the same body compiled for the host, on host memory, in the launch's order of
 * summation.  No HIP call; the same refusals.
 * mpg_*_ctl: the optimizer launches with lr = out[0] and gscale = out[1], read from device memory at the top of the kernel (the
 * arguments lr and gscale are not looked at); the per-element arithmetic is the plain launch's.  ema: NULL, or the averaged form's
 * block.  A NULL ctl or out, n == 0, a bad ema block: -1. */
#define MPG_LR_KNOTS 8
typedef struct MpgStepCtl {
    uint32_t* state;     /* t, ticket */
    float* base;
    float* out;          /* lr_eff, s, norm, factor */
    double* partials;    /* 256 doubles */
    int nknots;
    uint32_t knot_step[MPG_LR_KNOTS];
    float knot_f[MPG_LR_KNOTS];
    float max_norm;
    int want_norm;
} MpgStepCtl;
int mpg_step_control(const float* g, uint64_t n, float gscale, const MpgStepCtl* ctl, void* stream);
int mpg_step_control_host(const float* g, uint64_t n, float gscale, const MpgStepCtl* ctl);
int mpg_rmsprop_ctl(float* p, float* g, float* v, uint64_t n, float lr, float alpha, float eps, float gscale, int zero_grad,
                    uint64_t* counter, uint64_t counter_add, const MpgStepCtl* ctl, const MpgEma* ema, void* stream);
int mpg_adam_ctl(float* p, float* g, float* m, float* v, float* step, uint64_t n, float lr, float beta1,
                 float beta2, float eps, float weight_decay, float gscale, int zero_grad, uint64_t* counter, uint64_t counter_add,
                 const MpgStepCtl* ctl, const MpgEma* ema, void* stream);
int mpg_adadelta_ctl(float* p, float* g, float* v, float* u, uint64_t n, float lr, float rho, float eps,
                     float gscale, int zero_grad, uint64_t* counter, uint64_t counter_add, const MpgStepCtl* ctl, const MpgEma* ema,
                     void* stream);

/* ---- evaluation metrics --------------------------------------------------------------------------
 * mpg_jet_obs: per-jet observables of the metrics the reference's evaluate (train.py:543-606) draws from jetnet / energyflow:
 * jetnet.utils.jet_features (for w1m) and the EFPs of jetnet.evaluation.w1efp (energyflow ("n==",4), ("d==",4), ("p==",1)).
 * Particle p of jet b is (eta_rel, phi_rel, pt_rel) at jets[b*ld_jet + p*ld_part + 0..2] ([n, N, 3] or [n, N, 4] in place);
 * padding particles have pt_rel = 0, anywhere in the jet.  Each particle is a massless four-vector:
 *   kin[b] = (pt, eta, phi, mass) of their sum: pt = hypot(px, py), eta = asinh(pz / pt) (0 when pt = 0), phi = atan2(py, px),
 *            mass^2 = sum_{i,j} pT_i pT_j (cosh(eta_i - eta_j) - cos(phi_i - phi_j)) (not E^2 - |p|^2, which cancels in fp32);
 *   efp[b, k] (flags bit 0), hadronic measure, beta = 1: theta_ij = sqrt(d_eta^2 + d_phi^2), z_i = pT_i / sum pT (flags bit 1)
 *            or pT_i; sums over all index tuples; w = Theta z, u = (Theta o Theta) z, M = Theta diag(z) Theta:
 *            k = 0  a=b-c-d          sum_{b,c} z_b u_b theta_bc z_c w_c
 *            k = 1  a-b=c-d          sum_{b,c} z_b w_b theta_bc^2 z_c w_c
 *            k = 2  3-star, 1 double sum_c z_c u_c w_c^2
 *            k = 3  triangle+pendant sum_{a,c} z_a z_c w_c theta_ac M_ac
 *            k = 4  4-cycle          sum_{a,c} z_a z_c M_ac^2
 *            (this column order is the project's, not necessarily energyflow's).  A jet whose pT sum is 0 gives zeros.
 * 1 <= N <= MPG_JET_OBS_MAX_N (else -1).  fp32; fixed-order reductions: the same input gives the same bits. */
#define MPG_JET_OBS_MAX_N 160
#define MPG_JET_OBS_EFP 1
#define MPG_JET_OBS_NORMED 2
int mpg_jet_obs(const float* jets, int ld_jet, int ld_part, int n, int N, int flags, float* kin, float* efp, void* stream);

/* mpg_jet_efps_d4: efp[b, 0..20] = the 21 connected ("prime") energy-flow polynomials of degree <= 4 of jet b, the features of
 * FPD and KPD (jetnet.evaluation.fpd / kpd on jetnet.utils.efps(jets, efpset_args=[("d<=", 4)])).  energyflow's d<=4 set is
 * every loopless multigraph with at most 4 edges and no isolated vertex, up to isomorphism, the empty graph included: 36
 * graphs, of which these 21 are connected; the other 15 are disjoint unions, whose EFPs are the products of their components'
 * -- the caller multiplies (mpgan_amd/evaluation.py: EFP_D4_GRAPHS).  Input contract, measure and index conventions as for
 * mpg_jet_obs (theta_ij = sqrt(d_eta^2 + d_phi^2), z_i = pT_i / sum pT with MPG_JET_OBS_NORMED in flags, else pT_i; sums over
 * ALL index tuples, theta_ii = 0 removing the repeated ones; any other flag bit: -2).  With T_k = (Theta^{o k}) z, the row
 * sums of the k-th elementwise power (T_1 = w, T_2 = u), zw = z o w, v = Theta zw, q = (Theta o Theta) zw and
 * M = Theta diag(z) Theta:
 *   col  d  graph                                    closed form
 *    0   0  one vertex, no edge                      sum z            (1 when normed; 0 for a jet without pT)
 *    1   1  edge a-b                                 sum z w
 *    2   2  double edge a=b                          sum z T_2
 *    3   2  wedge a-b-c                              sum z w^2
 *    4   3  triple edge                              sum z T_3
 *    5   3  a=b-c                                    sum z T_2 w
 *    6   3  triangle                                 sum_{a,c} z_a z_c theta_ac M_ac
 *    7   3  path a-b-c-d                             sum zw v
 *    8   3  3-star                                   sum z w^3
 *    9   4  quadruple edge                           sum z T_4
 *   10   4  triple edge a-b + edge b-c               sum z T_3 w
 *   11   4  two double edges sharing b (a=b=c)       sum z T_2^2
 *   12   4  triangle, one edge doubled               sum_{a,c} z_a z_c theta_ac^2 M_ac
 *   13   4  a=b-c-d (end edge doubled)               sum z T_2 v            (= efp[b, 0] of mpg_jet_obs)
 *   14   4  a-b=c-d (middle edge doubled)            sum zw q               (= 1)
 *   15   4  3-star, one edge doubled                 sum z T_2 w^2          (= 2)
 *   16   4  triangle + pendant                       sum_{a,c} z_a z_c w_c theta_ac M_ac   (= 3)
 *   17   4  4-cycle                                  sum_{a,c} z_a z_c M_ac^2              (= 4)
 *   18   4  path of 5 vertices                       sum z v^2
 *   19   4  4-star                                   sum z w^4
 *   20   4  fork (3-star, one leg extended)          sum z w^2 v
 * (the column order is the project's; FPD and KPD do not depend on it).  Every summand is non-negative.  One launch, one
 * workgroup per jet, M one 32 x 32 tile at a time as in mpg_jet_obs; fp32; fixed-order reductions: the same input gives the
 * same bits.  1 <= N <= MPG_JET_OBS_MAX_N, n >= 1, ld_part >= 3 (else -1); jets, efp non-NULL (else -2). */
#define MPG_JET_EFPS_D4_PRIMES 21
int mpg_jet_efps_d4(const float* jets, int ld_jet, int ld_part, int n, int N, int flags, float* efp, void* stream);

/* mpg_jet_emd: out[i, j] = the energy mover's distance between jets a[i] and b[j] (i < na, j < nb), the pairwise distances
 * that jetnet.evaluation.cov_mmd takes from energyflow's emd (beta = 1, norm = False, no phi wrap).  Jets are laid out as for
 * mpg_jet_obs (particle p of jet i at a[i*ld_jet_a + p*ld_part + 0..2] = (eta_rel, phi_rel, pt_rel)); only particles with
 * pt_rel > 0 take part, wherever they sit in the jet.  With weights w_i = pT of a's particles, w'_j = pT of b's,
 * theta_ij = sqrt(d_eta^2 + d_phi^2) / R and d = sum w - sum w', the lighter jet gets one slack particle of weight |d| whose
 * cost to every particle of the other jet is exactly 1 (none when d == 0), and
 *   EMD(a, b) = min_{f >= 0} sum_ij f_ij cost_ij   subject to   sum_j f_ij = w_i,  sum_i f_ij = w'_j.
 * A jet without a particle of positive pT is all slack: EMD = sum pT of the other jet; two such jets give 0.
 * The solver is exact (successive shortest paths with potentials, csrc/jet_emd.hip), one launch for the whole matrix, fp32,
 * and out[i, j] depends on the values of a[i] and b[j] alone: equal jets give equal bits, in any position and on every launch.
 * status[i, j] (or NULL): 0, or 1 when the pair reached the solver's cap of 32 (N + 1) augmentations, 2 when a search found no
 * path (non-finite coordinates); out then holds the cost of a feasible plan, an upper bound.
 * 1 <= N <= MPG_JET_OBS_MAX_N, na, nb >= 1, R > 0, ld_part >= 3 (else -1). */
int mpg_jet_emd(const float* a, int ld_jet_a, const float* b, int ld_jet_b, int ld_part, int na, int nb, int N, float R,
                float* out, int* status, void* stream);
/* mpg_jet_emd_host: the same solver (the same code) in fp64 on host pointers, on min(threads, 16) std::threads; no HIP call.
 * mpg_jet_emd_host_iters also writes the augmentations each pair took (iters [na, nb] or NULL; the cap is 32 (N + 1)). */
int mpg_jet_emd_host(const float* a, int ld_jet_a, const float* b, int ld_jet_b, int ld_part, int na, int nb, int N, float R,
                     double* out, int* status, int threads);
int mpg_jet_emd_host_iters(const float* a, int ld_jet_a, const float* b, int ld_jet_b, int ld_part, int na, int nb, int N, float R,
                           double* out, int* status, int* iters, int threads);

/* The tag table.  Every family of draws hashes (seed or key, tag, ...) under tags of its own: MPG_x_TAG + a site or round number
 * below MPG_x_TAG_SPAN.  The spans are pairwise disjoint and lie at or above 2^27, the ceiling of the dropout sites' tags
 * (csrc/draws.h asserts both at compile time).
 *   NOISE    mpg_normal / mpg_normal_rank_mask: + the draw's site within an iteration (0 train_D's noise, 1 train_G's)
 *   AUG      mpg_augment: + the site (0 train_D's generated jets, 1 train_G's, 2 the gradient penalty's real jets)
 *   LABEL    mpg_label_targets: + the site (0)
 *   SHUFFLE  the keyed shuffle: + the Feistel round (0 .. 3)
 *   PICK     mpg_label_pick (0) */
#define MPG_NOISE_TAG 0x4E000000
#define MPG_NOISE_TAG_SPAN 0x100000
#define MPG_AUG_TAG 0x41000000
#define MPG_AUG_TAG_SPAN 0x100000
#define MPG_LABEL_TAG 0x4C000000
#define MPG_LABEL_TAG_SPAN 0x100000
#define MPG_SHUFFLE_TAG 0x53000000
#define MPG_SHUFFLE_TAG_SPAN 0x100000
#define MPG_PICK_TAG 0x50000000
#define MPG_PICK_TAG_SPAN 0x100000

/* mpg_normal: out[i] = mean + std * z_i with z ~ N(0, 1) -- the generator's input noise (get_gen_noise, train.py:100-141:
 * torch.randn * sd) from a counter-based stream keyed by the device-resident 64-bit `seed` (the dropout seed, advanced
 * once per iteration) and a site `tag`: a captured hipGraph draws fresh values on every replay, and torch's generator
 * (whose graph-safe state costs two fill launches in front of every replay) is not involved. */
int mpg_normal(float* out, uint64_t n, const uint64_t* seed, uint32_t tag, float mean, float std, void* stream);
/* mpg_normal_rank_mask: mpg_normal over a [B, N, L] noise tensor and mpg_rank_mask of its first feature (out[:, :, 0]) in one
 * launch -- same values, same masks; mask / ignore [B, N] (ignore = 1 - mask, or NULL), labels read at stride ld_lab.  N L even. */
int mpg_normal_rank_mask(float* out, int B, int N, int L, const uint64_t* seed, uint32_t tag, float mean, float std,
                         const float* labels, int ld_lab, float* mask, float* ignore, void* stream);

/* mpg_augment / mpg_augment_bwd: augment.augment (mpgan/augment.py; train_D / train_G, train.py:438-442, :508-511) on B jets
 * of N particles, F features each at row stride ld floats and jet stride jet_stride floats (the same for x and y: the second
 * half of a 2B-jet batch is a valid target).  All four stages are affine in (eta, phi) and act on a whole jet, so their
 * mixed composition is one map per jet,  y[b, i, 0:2] = A_b x[b, i, 0:2] + t_b;  columns >= 2 pass through (copied when
 * y != x; y may be x).  Padded particles are moved like the others, as the reference moves them.
 * Draws: word(i) = the project's counter-based hash of (the 64-bit *seed, tag, jet b, draw index i) -- the stream of the
 * dropout masks and of mpg_normal --, u(i) = (word(i) >> 8) * 2^-24 in [0, 1).  p is read from DEVICE memory (one float: a
 * captured hipGraph follows a changed probability without recapture); a stage is TAKEN iff its flag bit is set, p != 1 and
 * u(mix draw) < p -- p == 1 takes nothing, rand_mix's own quirk.  A stage whose bit is clear draws nothing.  Starting from
 * A = I, t = 0, in the reference's order:
 *   MPG_AUG_R90        mix u(0);  k = floor(4 u(1));  A <- R^k A, t <- R^k t,  R = [[0, -1], [1, 0]] (entries exactly 0 / +-1)
 *   MPG_AUG_FLIP       mix u(2);  s_eta = u(3) >= 0.5 ? +1 : -1, s_phi likewise from u(4);  A <- diag(s) A, t <- diag(s) t
 *   MPG_AUG_TRANSLATE  mix u(5);  t <- t + ((u(6), u(7)) - 0.5) * translate_ratio
 *   MPG_AUG_SCALE      mix u(8);  z = sqrt(-2 ln v(9)) cos(2 pi v(10)), v(i) = ((word(i) >> 8) + 0.5) * 2^-24 (mpg_normal's
 *                      form);  f = exp(scale_sd * z);  A <- f A, t <- f t
 * params [B, 6] receives (a00, a01, a10, a11, t0, t1) per jet.  N == 0 (x, y may be NULL): the maps alone.
 * mpg_augment_bwd: dx[b, i, 0:2] = A_b^T dy[b, i, 0:2] from the saved params, columns >= 2 copied; no random stream.
 * B >= 1, 2 <= F <= ld, jet_stride >= N ld (else -1). */
#define MPG_AUG_R90 1
#define MPG_AUG_FLIP 2
#define MPG_AUG_TRANSLATE 4
#define MPG_AUG_SCALE 8
int mpg_augment(const float* x, float* y, uint64_t jet_stride, int ld, int F, int B, int N, const uint64_t* seed, uint32_t tag,
                const float* p, int flags, float translate_ratio, float scale_sd, float* params, void* stream);
int mpg_augment_bwd(const float* dy, float* dx, uint64_t jet_stride, int ld, int F, int B, int N, const float* params,
                    void* stream);

/* mpg_label_targets: calc_D_loss's label smoothing and label noise (train.py:341-363; --label-smoothing / --label-noise,
 * setup_training.py:271-274) for the 2B jets of a D step, rows [0, B) the real half, as the per-jet targets and the scalar that
 * mpg_disc_head_loss / _bwd take (MpgDiscHead.targets, .loss_extra).  One workgroup; any B >= 1.
 * Draws: word(g) = the project's counter-based hash of (the 64-bit *seed, tag, jet b, group g) -- the stream of the dropout
 * masks, of mpg_normal and of the augmentation --, u_s = (word(0) >> 8) * 2^-24 and u_n = (word(1) >> 8) * 2^-24 in [0, 1).
 * tag = MPG_LABEL_TAG + site.
 *   Y_b = smoothing ? (real: 0.7f + 0.5f * u_s ~ U[0.7, 1.2);  generated: 0.3f * u_s ~ U[0, 0.3))  :  (real: 1;  generated: 0)
 *         -- one fp32 rounding each --, then, where u_n < noise, real: Y_b = 0, generated: Y_b = 1 (noise in [0, 1], else -1).
 * drawn [2B] (or NULL) receives Y.  What the loss makes of Y depends on its shape in the reference: without smoothing Y is
 * [B, 1] like D's outputs and the losses are per jet -- targets = Y, *extra = 0.  With smoothing Y is [B] and
 * MSELoss(out [B, 1], Y [B]) broadcasts to [B, B]:  mean_ij (out_i - Y_j)^2 = mean_i (out_i - mean(Y))^2 + popvar(Y)  per
 * half, so  targets[b] = the mean of Y over b's half  and  *extra = popvar(Y_real) + popvar(Y_generated)  (BCELoss refuses
 * those shapes: smoothing has a meaning for ls only).  Per half the mean first, then sum (Y - mean)^2 / B, both summed in one
 * fixed order (a thread's strided partial, a tree over the 256 partials); no atomics.  *seed is read from device memory: a
 * replayed hipGraph draws fresh labels. */
int mpg_label_targets(int B, int smoothing, float noise, const uint64_t* seed, uint32_t tag, float* targets, float* extra,
                      float* drawn, void* stream);

/* mpg_ada_update: the adaptive augmentation probability (--adaptive-prob, setup_training.py:399; the reference reads
 * augment_p[-1] under it, train.py:440, :510, and never fills it) -- ADA's rule (Karras et al. 2020) as ONE launch behind the D
 * step's head: mpg_augment's *p moved by the discriminator's outputs on the real jets.  One workgroup; csrc/ada.hip.
 * out [>= n_real] fp32: D's per-jet outputs of this D step, the real half first (MpgDiscHead.out); only out[0 .. n_real) is read.
 * mid: the midpoint of the loss's two targets (0.5 for og / ls, 0 for w / hinge).  state: int32[2] = {sign sum, D steps counted};
 * aug_p, r_out: one float each; all three in device memory.  One launch, all of it exact integer arithmetic up to the marked lines:
 *   s = #{b < n_real : out[b] > mid} - #{b < n_real : out[b] < mid}        (an output equal to mid, or a NaN, counts on neither side)
 *   state[0] += s;  state[1] += 1
 *   if state[1] == interval:
 *       r = (float) state[0] / (float) (n_real * interval)                 (two int32 -> fp32 conversions, ONE fp32 division)
 *       if r > target: p = *aug_p + step;  else if r < target: p = *aug_p - step;  else p = *aug_p     (ONE fp32 add / subtract)
 *       *aug_p = p < 0 ? 0 : (p > 1 ? 1 : p);  *r_out = r;  state[0] = state[1] = 0
 * Conversions, division and sum round to nearest even; nothing is contracted.  The sign counts are added as integers (a lane's
 * strided partial, shuffles within a wave, four words of LDS across the waves): the result does not depend on that order.  One
 * thread writes state, *aug_p and *r_out with ordinary stores: no atomics.  r = +1: every real jet of the interval scored on
 * the real side; p then moves by `step` towards 1 -- r > target says "D is overfitting, augment more".  A state whose count
 * already stands at or beyond `interval` never closes its interval: callers keep 0 <= state[1] < interval.
 * n_real < 1, n_real > 2^30, interval < 1, n_real * interval > 2^31 - 1, target outside [0, 1], step < 0 (a NaN in either), a
 * NULL pointer: -1.
 * mpg_ada_update_host: the same body compiled for the host on host memory, no HIP call. */
int mpg_ada_update(const float* out, int n_real, float mid, float target, float step, int interval, int32_t* state, float* aug_p,
                   float* r_out, void* stream);
int mpg_ada_update_host(const float* out, int n_real, float mid, float target, float step, int interval, int32_t* state,
                        float* aug_p, float* r_out);

/* mpg_ada_count / mpg_ada_settle: mpg_ada_update in two launches, for data-parallel ranks that settle ONE probability from the
 * sign sum of all their real jets.  The sum travels in the discriminator's gradient all-reduce: `slot` is one float at the tail
 * of the flat gradient buffer (TrainStep: FlatParams(tail=1)), no collective is added.
 * mpg_ada_count:   slot[0] = (float) s, s the count of mpg_ada_update over out[0 .. n_real) of THIS rank (an output equal to mid,
 *                  or a NaN, counts on neither side).  A store, not an add: what the slot held is gone.  One workgroup.
 *                  n_real < 1, n_real > 2^24, a NULL out or slot: -1.
 * mpg_ada_settle:  s = (int32) slot[0], then the rule of mpg_ada_update from `state[0] += s` onward with n_real_total -- the real
 *                  jets of all ranks -- in the division.  One thread.  If slot[0] is not an integer value (a NaN, an infinity, a
 *                  fraction) or |slot[0]| > n_real_total, the collective is broken: state and *aug_p stay untouched and
 *                  *r_out = NaN.  Refusals as mpg_ada_update's, with slot in out's place and n_real_total in n_real's.
 * The identity: mpg_ada_update(out, n, ...) leaves the same state, *aug_p and *r_out as mpg_ada_count(out, n, mid, slot)
 * followed by mpg_ada_settle(slot, n, ...), bit for bit.  With the outputs split over W ranks -- n = n_1 + ... + n_W <= 2^24 --
 * the W counts added in fp32 give (float) s in any order and any association: every partial sum is an integer of magnitude
 * <= 2^24, which fp32 holds exactly.  So every rank reads the same slot behind a SUM all-reduce and settles the same p.
 * mpg_ada_count_host / mpg_ada_settle_host: the same bodies compiled for the host on host memory, no HIP call. */
int mpg_ada_count(const float* out, int n_real, float mid, float* slot, void* stream);
int mpg_ada_count_host(const float* out, int n_real, float mid, float* slot);
int mpg_ada_settle(const float* slot, int n_real_total, float target, float step, int interval, int32_t* state, float* aug_p,
                   float* r_out, void* stream);
int mpg_ada_settle_host(const float* slot, int n_real_total, float target, float step, int interval, int32_t* state, float* aug_p,
                        float* r_out);

/* The keyed shuffle of a device-resident data set (csrc/shuffle.h: one body for the device and the host).
 * perm(key, epoch, i, n), 0 <= i < n <= 2^31 - 1, is a bijection of [0, n) computed from (key, epoch, i) alone -- a balanced
 * Feistel network with cycle walking, its round function the project's counter-based hash (the stream of the dropout masks, of
 * mpg_normal and of the augmentation draws):
 *   word(tag, row, grp) with the 64-bit key in place of the seed, lo = (uint32) key, hi = (uint32) (key >> 32), all in uint32:
 *       x = (row + lo) * 0x9E3779B1;  x ^= (grp + tag * 0x10001) * 0x85EBCA77 + hi;
 *       x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *   n == 1: perm = 0.  Otherwise k = the bit length of n - 1, h = (k + 1) / 2 (integer division), m = 2^h - 1: the domain is
 *   [0, 2^(2h)), 2^(2h) < 4 n.  Starting from x = i:
 *       L = x >> h, R = x & m;
 *       four rounds r = 0, 1, 2, 3:  (L, R) <- (R, L ^ (word(MPG_SHUFFLE_TAG + r, R, (uint32) epoch) & m));
 *       x = (L << h) | R;
 *   again from the new x while x >= n (the walk); perm = the first x < n.  Only the low 32 bits of the epoch enter.
 * The stream is continuous: position g = 0, 1, 2, ... takes data-set row perm(key, g / n, g % n, n).  No batch is dropped or
 * short, a batch may straddle two epochs, and every n consecutive positions from a multiple of n visit every row once.
 *
 * mpg_shuffle_index_host: out[c] = the row of position pos0 + c, c < count; no HIP call.  1 <= n <= 2^31 - 1, count >= 0 (else -1). */
int mpg_shuffle_index_host(uint64_t key, uint64_t pos0, int64_t count, int64_t n, int32_t* out);

/* mpg_batch_feed: one training batch gathered from the resident data set -- normalised particles [n, N, 4] fp32 (a particle row
 * is one 16-byte-aligned float4) and labels_in [n] -- in ONE launch: jet j < B takes position *cursor + j of the stream above.
 * With v = the jet's particle rows, m = v[:, 3] and l = its label, the launch writes what TrainStep.set_batch writes, bit for bit:
 *   data [B, N, 4] = v;  labels [B] = l;  dcat[:B] = v ([*, N, 4]);  x3[:B] = v[:, 0:3] ([*, N, 3]);  mask2[:B] = m + 0.5f and
 *   ign2[:B] = 0.5f - m ([*, N]);  labels2[j] = labels2[B + j] = l ([2B]).
 * Any output may be NULL (labels_in too, when labels and labels2 are).  The same launch then moves *cursor on by `stride` (a
 * rank of W strides by W B), behind every workgroup's read of it: the workgroup that arrives last on the agent-scope counter
 * *ticket does it and leaves the counter at zero, as it found it (no second kernel).  *cursor and *ticket live in device memory.
 * n < 1, n > 2^31 - 1, B < 1, N < 1, a NULL cursor, ticket or data set: -1; particles, data or dcat off a 16-byte boundary: -2. */
int mpg_batch_feed(const float* particles, const float* labels_in, int64_t n, int N, uint64_t key, uint64_t* cursor,
                   uint32_t* ticket, int B, uint64_t stride, float* data, float* labels, float* dcat, float* x3, float* mask2,
                   float* ign2, float* labels2, void* stream);

/* Bulk generation as a stream of rows (gen.JetSampler; csrc/sampler.hip).  Row g = 0, 1, 2, ... of the stream is one generated
 * jet; a launch of B jets (one CHUNK; B is fixed for a stream) covers rows *cursor .. *cursor + B - 1, and chunk c = rows
 * c B .. c B + B - 1.  Everything a row holds is a function of (key, g) and the generator's weights:
 *   its label   table[idx(g)],  idx(g) = ((uint64) word(MPG_PICK_TAG, (uint32) g, (uint32) (g >> 32)) * n) >> 32,  word the
 *               project's counter-based hash as the keyed shuffle above spells it out, with the 64-bit key in place of the seed.
 *               This is rng.choice(len(labels), size) of the reference's gen.py:105-107 as a keyed stream: a draw with
 *               replacement from table [n], the data set's num_particles / N.  The multiply-shift is not exactly uniform:
 *               an index is taken by floor(2^32 / n) or that plus one of the 2^32 words, a relative bias below n / 2^32.
 *   its noise   drawn by mpg_normal / mpg_normal_rank_mask under the seed word of its chunk,
 *               seed_c = key + c * 0x9E3779B97F4A7C15 (mod 2^64), at the row's place within the chunk.
 * So the labels are a function of the row alone, the noise of (chunk index, place in the chunk): the same key and B give the
 * same jets whatever ran before, and any row can be recomputed.
 *
 * mpg_label_pick: labels[b] = table[idx(*cursor + b)], b < B; table, *cursor and labels in device memory; the cursor is only
 * read.  n < 1, n > 2^31 - 1, B < 1, a NULL table, cursor or labels: -1.
 * mpg_label_pick_host: out[c] = idx(pos0 + c), c < count -- the same body compiled for the host, no HIP call.
 * 1 <= n <= 2^31 - 1, count >= 0, out non-NULL when count > 0 (else -1). */
int mpg_label_pick(const float* table, int64_t n, uint64_t key, const uint64_t* cursor, int B, float* labels, void* stream);
int mpg_label_pick_host(uint64_t key, uint64_t pos0, int64_t count, int64_t n, int32_t* out);

/* mpg_jets_finish: the epilogue of the reference's gen.py:127-141 for one chunk, written into the final array.
 * feat: the chunk's particle rows [B N, >= 3] at row stride ld_feat floats, past the generator's final activation
 * (generate_parts(feat_out=...): ld_feat 3; a module's [B, N, 4] output: ld_feat 4).  mask [B, N] (1 real, 0 padded) or NULL
 * for "all real".  maxes, norms, shifts: three floats each in HOST memory, read at the call (data.FEATURE_MAXES[jet_type],
 * FEATURE_NORMS, FEATURE_SHIFTS).  out [total, N, 3] and mask_out [total, N] (or NULL) in device memory.
 * Jet b < B is stream row g = *cursor + b and row r = g - row0 of out (row0: the stream row at which the caller's array
 * begins; uint64 arithmetic).  r >= total: nothing is written for the jet -- the last chunk of a call may be short.  Otherwise,
 * per particle i, with x = its feature row and m = mask[b, i]:
 *   real = mask == NULL or (m - 0.5f) >= 0.5f          (gen.py's gen_jets[:, :, -1] >= 0.5 on the generator's mask - 0.5 column)
 *   v_f  = real ? ((x_f - shift_f) / norm_f) * max_f : 0,  f = 0, 1, 2: a subtraction, a division and a product, each rounded
 *          to fp32 on its own, in data.unnormalise_jets' order (nothing contracted);  then v_2 = v_2 < 0 ? 0 : v_2
 *   out[r, i, :] = v;  mask_out[r, i] = real ? 1 : 0.
 * One thread per particle; rows of out are 12 bytes: no alignment beyond a float's is assumed of out, feat or the masks.
 * The same launch then moves the stream on, behind every workgroup's read of the cursor, as mpg_batch_feed does: the workgroup
 * that arrives last on the agent-scope counter *ticket writes  *cursor += B,  *seed = key + (new cursor / B) * 0x9E3779B97F4A7C15
 * (mod 2^64: the seed word seed_c of the next chunk) and leaves *ticket at zero, as it found it.  *cursor, *seed and *ticket
 * live in device memory.  B < 1, N < 1, total < 0, ld_feat < 3, a NULL feat, out, cursor, seed, ticket, maxes, norms or
 * shifts: -1. */
int mpg_jets_finish(const float* feat, int ld_feat, const float* mask, int B, int N, const float* maxes, const float* norms,
                    const float* shifts, float* out, float* mask_out, uint64_t row0, int64_t total, uint64_t key, uint64_t* cursor,
                    uint64_t* seed, uint32_t* ticket, void* stream);

/* mpg_jets_finish_stride: mpg_jets_finish for a rank of W data-parallel ranks that share ONE stream (gen.JetSampler(rank=,
 * world_size=)): chunk c of the global stream goes to rank c mod W, so a rank's cursor starts at rank * B and the launch moves
 * it by stride = W B:  *cursor += stride,  *seed = key + (new cursor / B) * 0x9E3779B97F4A7C15 (mod 2^64) -- the seed word of
 * the rank's next chunk of the global stream.  Everything else, the row arithmetic included, is mpg_jets_finish: the caller
 * passes each launch the row0 that lands the chunk at its place in the rank's own array.  mpg_jets_finish is this entry with
 * stride = B.  stride < 1: -1. */
int mpg_jets_finish_stride(const float* feat, int ld_feat, const float* mask, int B, int N, const float* maxes, const float* norms,
                           const float* shifts, float* out, float* mask_out, uint64_t row0, int64_t total, uint64_t key,
                           int64_t stride, uint64_t* cursor, uint64_t* seed, uint32_t* ticket, void* stream);

/* ---- spectral normalisation of Linear layers (mpgan/spectral_normalization.py:29-46), grouped; csrc/spectral.hip ----------------
 * One job per wrapped layer, one workgroup per job, up to MPG_SPECTRAL_MAX_JOBS jobs per launch.  Everything is fp32 and
 * contiguous (W, W_eff, G, dW row-major [R, C]); no alignment beyond a float's is assumed: W is a view into a flat parameter buffer.
 *
 * mpg_spectral_norm, per job, with P = power_iterations >= 0, u' = u and v' = v to start with:
 *   P times:   t = W^T u';  v' = t / (||t||_2 + 1e-12);  s = W v';  u' = s / (||s||_2 + 1e-12)
 *   sigma = u' . (W v')                 (P >= 1: W v' is the s of the last pass; P = 0: formed from u and v as they stand)
 *   inv = 1 / (sigma + 1e-12);  W_eff = W * inv;  u_out = u';  v_out = v';  *inv_sigma = inv
 *   P >= 1:    u = u', v = v' stored in place, at the caller's (the parameters') own addresses, last of all; P = 0 writes neither.
 * u_out, v_out and inv_sigma are fresh copies for the backward: a later launch that moves u and v on does not touch them.
 * Every sum -- the two products, the two norms, the dot product -- is added in a fixed order (a lane's strided partial, shuffles
 * within a wave, the waves' partials in wave order): no atomics, the same bits on every run from the same inputs.
 * -1: a NULL pointer, R < 1, C < 1, P < 0, njobs outside [1, MPG_SPECTRAL_MAX_JOBS];  -2: two jobs of the launch name the same u or
 * the same v;  -3: u_out == u or v_out == v.
 *
 * mpg_spectral_norm_bwd, per job: the gradient with respect to W of a loss whose gradient with respect to W_eff is G, with u_out and
 * v_out constants of the differentiation (as the reference's wrapper has them: they are .data there):
 *   dW (+)= (G - <G, W_eff> u v^T) * inv_sigma,   <G, W_eff> = sum_ij G_ij W_eff_ij,   (+)= when accumulate, = otherwise
 * (u, v, inv_sigma: the forward's u_out, v_out, inv_sigma).  -1: a NULL pointer, R < 1, C < 1, njobs out of range.
 *
 * mpg_spectral_norm_host / mpg_spectral_norm_bwd_host: the same per-layer routines compiled for the host, on host memory, one job
 * after the other; no HIP call. */
#define MPG_SPECTRAL_MAX_JOBS 16
typedef struct MpgSpectralJob {
    const float* W; float* u; float* v;
    float* W_eff; float* u_out; float* v_out; float* inv_sigma;
    int R, C;
} MpgSpectralJob;
typedef struct MpgSpectralBwdJob {
    const float* G; const float* W_eff; const float* u; const float* v; const float* inv_sigma;
    float* dW;
    int R, C, accumulate;
} MpgSpectralBwdJob;
int mpg_spectral_norm(const MpgSpectralJob* jobs, int njobs, int power_iterations, void* stream);
int mpg_spectral_norm_bwd(const MpgSpectralBwdJob* jobs, int njobs, void* stream);
int mpg_spectral_norm_host(const MpgSpectralJob* jobs, int njobs, int power_iterations);
int mpg_spectral_norm_bwd_host(const MpgSpectralBwdJob* jobs, int njobs);

/* ---- set-pooling baselines: the last per-particle layer and the pooling over a jet's particles in one launch ----------------------
 * mpg_point_pool_fwd replaces  torch.max(sfc(x).reshape(-1, num_hits, C), 1)[0]  of rGAND (ext_models/ext_models.py:70-71) and
 * pointfc's last layer with  torch.cat((torch.max(x, dim=1)[0], torch.mean(x, dim=1)), dim=1)  of PointNetMixD
 * (ext_models/ext_models.py:203-206).  For jet b < B, particle n < N, channel c < C:
 *     z = sum_k x[(b N + n) ldx + k] W[c ldw + k] + bias[c]        (bias NULL = 0),      y = act ? LeakyReLU_alpha(z) : z
 *     mode bit 0:  pooled[b ld_pooled + c] = max_n y;   argmax[b C + c] (int32, where non-NULL) = the lowest n that attains it
 *     mode bit 1:  pooled[b ld_pooled + (mode & 1 ? C : 0) + c] = (sum_n y) / N          (torch.cat((max, mean), 1)'s order)
 *     neg (where non-NULL): bit (c & 31) of word neg[(b N + n) ceil(C / 32) + (c >> 5)] is set where !(z > 0) -- the slope
 *     torch's leaky_relu_backward takes; bits of columns >= C are clear.
 * With argmax and neg NULL neither is written.  The [B N, C] activation is never written: it lives in MFMA accumulators (particles
 * as rows, channels as columns: the pooling is an in-lane reduction).  Products as every forward product: fp16 hi / lo operands,
 * three terms, fp32 accumulate, no operand scales (mpg_gemm's f16 range); the bias is added in fp32.  Reductions run in a fixed order
 * (csrc/point_pool.hip): a jet's results depend neither on B nor on the grid nor on the run.  Nothing is read beyond K columns of a
 * row of x or W.
 * mpg_point_pool_bwd expands gpooled = dL/dpooled [B, ld_gpooled] into the pre-activation's gradient (element-wise, no reduction):
 *     dz[(b N + n) ld_dz + c] = slope (gmax[b,c] [n == argmax[b,c]] + gmean[b,c] / N),   slope = act ? (bit ? alpha : 1) : 1
 * from which dx = dz W, dW = dz^T x and db = colsum dz are ordinary mpg_gemm launches.  It reads argmax (mode bit 0) and neg (act).
 * Limits: B >= 1, 1 <= N <= MPG_POINT_POOL_MAX_N, 1 <= K <= MPG_POINT_POOL_MAX_K (fwd), 1 <= C <= MPG_POINT_POOL_MAX_C; unit column
 * stride, ldx, ldw >= K, ld_pooled, ld_gpooled >= the pooled width, ld_dz >= C; 0 <= alpha <= 1; f16 = 1 (the bf16 form is not built).
 * Errors, before the first HIP call: -1 a size outside the limits, -3 mode not in {1, 2, 3}, -4 alpha, -6 f16 != 1, -2 a NULL
 * x / W / pooled (fwd), gpooled / dz / needed argmax / needed neg (bwd), -5 a stride below its row. */
#define MPG_POINT_POOL_MAX_N 160
#define MPG_POINT_POOL_MAX_K 256
#define MPG_POINT_POOL_MAX_C 1024
typedef struct MpgPointPool {
    const float* x; int ldx; const float* W; int ldw; const float* bias;
    int B, N, K, C;
    int act; float alpha; int mode, f16;
    float* pooled; int ld_pooled; int* argmax; unsigned int* neg;
    const float* gpooled; int ld_gpooled; float* dz; int ld_dz;
} MpgPointPool;
int mpg_point_pool_fwd(const MpgPointPool* p, void* stream);
int mpg_point_pool_bwd(const MpgPointPool* p, void* stream);

/* ---- TreeGAN generator: one TreeGCN layer (ext_models/ext_models.py:211-282) in one launch per direction ---------------------------
 * Layer d of the tree has P parent nodes of width in, each with g children of width out.  level[i] = tree[i], contiguous
 * [B, nodes[i], width[i]] for i = 0 .. d (nodes[0] = 1 and level[0] the noise in the generator; nodes[d] = P, width[d] = in); the
 * ancestor of node p on level i is anc_i(p) = p / (P / nodes[i]) -- the reference's repeat / view.  For jet b < B, node p < P,
 * child c = p g + j (j < g):
 *     root[b,p]   = sum_{i<=d} level[i][b, anc_i(p), :] W_root[i]^T                      W_root[i]: [out, width[i]] contiguous
 *     u[b,c,:]    = LeakyReLU_alpha(level[d][b,p,:] W_branch[p])[j in : (j+1) in]        W_branch: [P, in, g in] contiguous
 *     h[b,c,:]    = u[b,c,:] Wc^T + root[b,p]                                            Wc = W_loop.1 W_loop.0: [out, in] contiguous
 *     y[(b P g + c) ld_y + o] = act ? LeakyReLU_alpha(h + bias[j out + o]) : h + bias[j out + o]        (bias [g, out]; NULL = 0)
 *     u[(b P g + c) ld_u + k]  is written where u != NULL (what the backward reads); with u NULL nothing is written for it.
 * The reference's [rows, in support] activation of W_loop is never formed: Wc comes from a GEMM in front of this launch.  Products:
 * fp16 hi / lo operands, three terms, fp32 accumulate (mpg_gemm's f16 range).  Sums run in a fixed order (csrc/tree_gcn.hip; no
 * atomics): a jet's values depend neither on B, nor on its position in the batch, nor on the grid, nor on the run.  Nothing is read
 * or written beyond the live rows, columns and k.
 * mpg_tree_gcn_bwd, given dy = dL/dy [(b P g + c) ld_dy + o], the stored y (act only) and u, writes the data side:
 *     dz[(b P g + c) ld_dz + o] = dy (act ? (y > 0 ? 1 : alpha) : 1)
 *     S[(b P + p) out + o]      = sum_j dz[b, p g + j, o]                                 (j ascending)
 *     du[(b P g + c) in + k]    = (dz[b,c,:] Wc)[k] (u[b,c,k] > 0 ? 1 : alpha)            (bf16 hi / lo, three terms)
 *     dx[(b P + p) in + k]      = du[b,p,:] W_branch[p]^T                                 (dx != NULL; the branch's share of dtree[d])
 * from which db = colsum dz, M = dz^T u (dW_loop.0 = W_loop.1^T M, dW_loop.1 = M W_loop.0^T), dW_branch[p] = level[d][:,p]^T du[:,p],
 * S_i = the sums of S over the descendants of a level-i node, dW_root[i] = S_i^T level[i] and dtree[i] += S_i W_root[i] are mpg_gemm
 * launches.  It reads no level and no W_root.
 * Limits: B >= 1; 0 <= d < MPG_TREE_GCN_MAX_LEVELS; 1 <= in, out, width[i] <= MPG_TREE_GCN_MAX_WIDTH; g >= 1, g in <=
 * MPG_TREE_GCN_MAX_BRANCH; P g <= MPG_TREE_GCN_MAX_NODES; P a multiple of every nodes[i]; ld_y, ld_dy, ld_dz >= out, ld_u >= in;
 * 0 <= alpha <= 1.
 * Errors, before the first HIP call: -1 a size outside the limits, -3 node counts that do not nest (or width[d] != in, nodes[d] != P),
 * -4 alpha, -2 a NULL descriptor / level / W_root / W_branch / Wc / y (fwd), W_branch / Wc / u / dy / dz / S / du / needed y (bwd),
 * -5 a stride below its row. */
#define MPG_TREE_GCN_MAX_LEVELS 8
#define MPG_TREE_GCN_MAX_WIDTH 128
#define MPG_TREE_GCN_MAX_BRANCH 256
#define MPG_TREE_GCN_MAX_NODES 160
typedef struct MpgTreeGcn {
    const float* level[MPG_TREE_GCN_MAX_LEVELS]; const float* W_root[MPG_TREE_GCN_MAX_LEVELS];
    int width[MPG_TREE_GCN_MAX_LEVELS]; int nodes[MPG_TREE_GCN_MAX_LEVELS];
    const float* W_branch; const float* Wc; const float* bias;
    int B, P, g, in, out, d;
    int act; float alpha;
    float* y; int ld_y; float* u; int ld_u;
    const float* dy; int ld_dy; float* dz; int ld_dz;
    float* S; float* du; float* dx;
} MpgTreeGcn;
int mpg_tree_gcn_fwd(const MpgTreeGcn* p, void* stream);
int mpg_tree_gcn_bwd(const MpgTreeGcn* p, void* stream);

/* ---- PCGAN's set encoder: the equivariant stack phi and the max over a jet's particles in one launch ------------------------------
 * (ext_models/pcgan_model.py:4-42 PermEqui1_max / PermEqui2_max / PermEqui2_mean behind a Tanh or a Softplus, :89-91 / :140-142 the
 * max.)  For jet b < B with particles n < N: h_0 = x[(b N + n) ldx + k], k < K[0]; for layer l < L, with Gamma[l] [D[l], K[l]] and
 * Lambda[l] [D[l], K[l]] contiguous (the modules' raw fp32 weights: nothing is cached on the host, a captured launch follows
 * in-place weight updates), bias[l] [D[l]] (NULL = 0), and m = the column-wise max_n h_l (pool 1, 2) or (sum_n h_l) / N (pool 3;
 * the sum in ascending n):
 *     pool 1 (max1):            z = (h_l - m) Gamma[l]^T + bias[l]         (the subtraction in fp32, in front of the operand split)
 *     pool 2 (max), 3 (mean):   z = h_l Gamma[l]^T + bias[l] - m Lambda[l]^T
 *     h_{l+1} = act(z):  act 2 tanh, act 3 torch's Softplus (z > 20 ? z : log1p(exp(z)))
 *     pooled[b ld_pooled + c] = max_n h_L[n, c],  c < D[L-1]
 * No [B N, D] activation is written: a group of jets (128 / (32 ceil(N / 32)) of them) stays in LDS for the whole stack
 * (csrc/set_encode.hip).  Products: fp16 hi / lo operands, three terms, fp32 accumulate.  Reductions run in fixed orders without
 * atomics: a jet's bits depend neither on B, nor on its position in the batch, nor on the grid, nor on the run.  Nothing is read
 * beyond K[0] columns of a row of x, beyond N rows of a jet or beyond the weights' extents; only pooled[b, c < D[L-1]] is written.
 * Forward only (the reference runs this encoder frozen, train.py:837-839).
 * Limits: B >= 1; 1 <= N <= MPG_SET_ENC_MAX_N (a jet's rows of 256 fp32 columns must fit the CU's LDS beside the other jets' --
 * 128 rows are 130 KiB of 160); 1 <= L <= MPG_SET_ENC_MAX_LAYERS; 1 <= K[0], D[l] <= MPG_SET_ENC_MAX_D; K[l+1] == D[l].
 * Errors, before the first HIP call: -1 a size outside the limits or widths that do not chain, -3 pool not in {1, 2, 3} or act not in
 * {2, 3}, -2 a NULL descriptor / x / pooled / Gamma[l] / (pool 2, 3) Lambda[l], -5 ldx < K[0] or ld_pooled < D[L-1]. */
#define MPG_SET_ENC_MAX_N 128
#define MPG_SET_ENC_MAX_D 256
#define MPG_SET_ENC_MAX_LAYERS 4
typedef struct MpgSetEncode {
    const float* x; int ldx;
    int B, N, L, pool, act;
    int K[MPG_SET_ENC_MAX_LAYERS]; int D[MPG_SET_ENC_MAX_LAYERS];
    const float* Gamma[MPG_SET_ENC_MAX_LAYERS]; const float* bias[MPG_SET_ENC_MAX_LAYERS]; const float* Lambda[MPG_SET_ENC_MAX_LAYERS];
    float* pooled; int ld_pooled;
} MpgSetEncode;
int mpg_set_encode_fwd(const MpgSetEncode* p, void* stream);

/* ---- GraphCNN-GAN generator: one edge-conditioned convolution (PyG's NNConv, aggr = "mean", root_weight, bias; ----------------------
 * ext_models/ext_models.py:75-157) on a k-nearest-neighbour graph, without a weight matrix per edge.
 * x is [B N, Cin] with row stride ld_x; nbr the [B N][ceil(N / 32)] words of mpg_knn_sets (bit j of row (b, i) set <=> node j of
 * jet b is a neighbour of receiver i; bits beyond N are ignored); nn_weight [Cin Cout, Cin], nn_bias [Cin Cout], root [Cin, Cout],
 * bias [Cout] are the module's raw contiguous fp32 parameters (PyG 1.x layouts: nothing is repacked or cached on the host, a
 * captured launch follows in-place weight updates).  With N(i) the set bits of row i in ascending j, n_i their number:
 *     P_i[c,d] = (1 / n_i) sum_{j in N(i)} x_j[c] (x_j[d] - x_i[d])        m_i[c] = (1 / n_i) sum_{j in N(i)} x_j[c]
 *     y[(b N + i) ld_y + o] = sum_{c,d} P_i[c,d] nn_weight[(c Cout + o) Cin + d] + sum_c m_i[c] nn_bias[c Cout + o]
 *                             + sum_c x_i[c] root[c Cout + o] + bias[o]
 * which equals mean_j x_j ((nn_weight (x_j - x_i) + nn_bias).view(Cin, Cout)) + x_i root + bias.  A row without a set bit has
 * P = m = 0 (a zero message).  The differences are taken in fp32 in front of every product and of the operand split; the product
 * with [W3 ; Bn ; root] takes fp16 hi / lo operands, three terms, fp32 accumulate (mpg_gemm's f16 range, for |P| as for x).
 *     pm[(b N + i) Cin (Cin + 1) + c Cin + d] = P_i[c,d],  pm[.. + Cin Cin + c] = m_i[c]   where pm != NULL (fwd), else not written.
 * mpg_nnconv_bwd, given dy = dL/dy [(b N + i) ld_dy + o] and the parked pm, writes into the workspace g [B N, Cin (Cin + 1)]
 *     G_i[c,d] = sum_o dy_i[o] nn_weight[(c Cout + o) Cin + d]   and   dm_i[c] = sum_o dy_i[o] nn_bias[c Cout + o]   (behind G_i)
 * and from them, in a second launch behind the first,
 *     dx[(b N + j) ld_dx + c] = sum_o dy_j[o] root[c Cout + o] - sum_c' G_j[c',c] m_j[c']
 *                               + sum_{i : j in N(i)} (1 / n_i) (dm_i[c] + sum_d G_i[c,d] (x_j[d] - x_i[d]) + sum_c' x_j[c'] G_i[c',c])
 * in fp32 (the listing receivers i ascending).  The parameter gradients are GEMMs of pm, x and dy: d nn_weight[c Cout + o, d] =
 * sum_i P_i[c,d] dy_i[o], d nn_bias[c Cout + o] = sum_i m_i[c] dy_i[o], d root = x^T dy, d bias = colsum dy.  The neighbour
 * sets carry no gradient.  Every sum runs in a fixed order without atomics (csrc/nnconv.hip): a jet's values depend neither on
 * B, nor on its position in the batch, nor on the run.  Nothing is read or written beyond the live rows and columns.
 * Limits: 1 <= B <= MPG_NNCONV_MAX_B; 1 <= N <= MPG_NNCONV_MAX_N; 1 <= Cin, Cout <= MPG_NNCONV_MAX_C.
 * Errors, before the first HIP call: -1 a size outside the limits, -2 a NULL descriptor / x / nbr / parameter / y (fwd) / pm, dy,
 * g, dx (bwd), -5 a stride below its row. */
#define MPG_NNCONV_MAX_N 160
#define MPG_NNCONV_MAX_C 64
#define MPG_NNCONV_MAX_B (1 << 20)
typedef struct MpgNNConv {
    const float* x; int ld_x;
    const unsigned int* nbr;
    const float* nn_weight; const float* nn_bias; const float* root; const float* bias;
    int B, N, Cin, Cout;
    float* y; int ld_y;
    float* pm;
    const float* dy; int ld_dy;
    float* g;
    float* dx; int ld_dx;
} MpgNNConv;
int mpg_nnconv_fwd(const MpgNNConv* p, void* stream);
int mpg_nnconv_bwd(const MpgNNConv* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPGAN_AMD_H */
