// dpmm_kernels.h -- kernel argument blocks and host-side launchers (internal to libdpmmhip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "stats_ranges.h"

#define DPMM_MAX_CLUSTERS_K 1024

namespace dpmm {

// Device-resident label state: bins[i] = 2*(label-1) + (sub_label-1)  (Int32).
// The (label, sub-label) pair of the reference (src/ds.jl:54-55) is exactly the
// sufficient-statistics bin the point contributes to.

constexpr int DPMM_WORK_QUEUES = 8;                               // queue heads of the D <= 64 sweep kernel, 16 u64 apart from work[8]
constexpr int DPMM_WORK_SLOTS = 8 + 16 * DPMM_WORK_QUEUES;        // first per-wave counter slot
constexpr int DPMM_WORK_PER_WAVE = 8;                             // u64 per wave slot (one 64-byte half line): wave tiles, full evaluations, 16-row screens, tail pairs, reference brackets, 3 spare
constexpr int REFB_FRAGS = 6, REFB_WORDS = REFB_FRAGS * 256;      // dwords of a cluster's bf16 image for the reference bracket (refb_map, dpmm_device.h)
constexpr int B3_WORDS = 3 * REFB_WORDS;                           // dwords of a matrix's three-plane bf16 image (planes h | m | l, each in the bracket's fragment layout): niw_lean.hip
constexpr int B3_DVEC = 64;                                        // floats of a sub-cluster's offset vector d = R_s (mu_k - mu_s)

// The flag bits of NiwSweepArgs::ball and ::bf16scr.  They share two ints because the block's layout is frozen (see the static_asserts behind it).
enum NiwBall : int {
    NIW_BALL_ON = 1,            // cluster-per-lane ball test in front of the per-point tail screen (records [K][16] behind the pair records)
    NIW_BALL_PAIR_TABLE = 2,    // lean launch: the pair-ball table of niw_pair_ball_kernel belongs to these parameters
    NIW_BALL_NORM_CERT = 4,     // lean launch: the norm certificate runs (DPMM_OPT_LEAN_NORM_CERT)
    NIW_BALL_NB_LOOSE = 8,      // ... and the neighbours keep the loose norm sn in its comparison (DPMM_OPT_LEAN_NORM_CERT = 3)
};
enum NiwScreens : int {
    NIW_SCR_ON = 1,             // D in 33..64 with tail records: bf16 screens in front of the Float32 16-row screen and of every survivor's first row block (DPMM_OPT_BF16_SCREENS)
    NIW_SCR_DIR_FIRST = 2,      // (with sp_frag): the direction screen runs in FRONT of the tail-pair tests (the sweeps between two measuring ones)
};

// THE RULE of this block: its size and every offset are frozen (static_asserts below).  A slot that means something else in another launch gets a
// union member and a name of its own -- never a cast, never a new field.
struct NiwSweepArgs {
    const float *X;      // [n][ldx] points (zero padded to ldx = roundup(D,4))
    int64_t ldx;
    int64_t n;
    int64_t first_index; // global index of point 0 (RNG counter)
    int64_t ntiles;
    int K;
    const float *Rp;     // packed factor fragments [3K][NP][64][4]
    const float *mup;    // [3K][DP]
    const float *cst;    // [3K]: 3k: -logdet/2 + log w_k ; 3k+1+s: -logdet/2 + log lr_w[k][s]
    union {
        const float *tdf;           // null: Gaussian a = cst - q/2 ; else Student-t (posterior predictive): [3K][2] = {df, (df+D)/2}, a = cst - hdf*log1p(q/df)
        const uint32_t *tile_list;  // label-storing launches (NiwLabelStore; no Student-t mode there): [0] = count, [1 ..] = the spans to walk; null: all tiles
    };
    float *scratch;      // a_k rows: scratch[k*scratch_stride + base + point_in_tile]
    int64_t scratch_stride;
    int scratch_by_tile; // 1: base = tile*TILE (full table, debug) ; 0: base = blockIdx*TILE
    int labels_only;     // 1: stop after the label phase (debug_loglik)
    int32_t *bins;       // out
    const int32_t *order_total; // device scalar: number of points `order` covers (must equal n, else identity is used)
    const int32_t *order; // processing order (permutation of [0,n), e.g. sorted by the previous bins) or null = identity
    uint64_t seed;
    uint32_t epoch;
    int final_argmax;
    float screen_margin;      // > 0: skip clusters whose a_k is provably below (reference - margin) for a whole wave (NIW, D in 17..64)
    const float *tail;        // [ceil(K/2)][16][2] tail-screen records of the cluster-level matrices, pairs interleaved, then [K][16] ball records (null: no tail screen)
    int tail_g;               // row group (lane >> 4) whose x registers of the last block hold features D-4..D-1
    int ball;                 // NiwBall bits
    int bf16scr;              // NiwScreens bits
                              // (A field of its own for NIW_SCR_DIR_FIRST cost the common kernel 32 spilled registers: the argument block's size decides how the compiler lays out its scalars.)
    int bracket;              // 1: D in 33..64, homogeneous waves: certified bf16 bracket of the reference cluster's value first; its Float32 evaluation only if a cluster survives the screens (bf16 images behind the ball records)
    const float *lam;         // [K] lower bounds of lambda_min(Sigma_k^-1) (null: no scalar pre-screen)
    union {
        const float *mdist;   // [K][K] distances between the cluster means (the scalar pre-screen's table: read only with lam)
        uint32_t *list_len;   // launches that walk a tile_list (lam is null there): pinned host word that receives the list's length (nullable)
    };
    int screen_lds;           // set by the launcher: screen operands of all K clusters are staged in LDS
    int use_prev;             // bins hold labels from a previous sweep (reference clusters of the screen)
    int lds_rows;             // set by the launcher: rows of the a_k table that live in LDS (0: global scratch)
    union {
        const uint32_t *sp_frag;   // direction screen (D in 33..64, K <= 64; null: none): [K][4][2][64][4] bf16 fragments of the pair directions w, k0 major (launch_niw_direction)
        const uint32_t *brk_flag;  // D = 128, 256: one word per 128-point tile, 1 + k0 where launch_niw_bracket_big bracketed the tile's reference cluster, else 0 (null: none)
    };
    union {
        const float *sp_cons;      // [K][3][64]: per reference cluster k0 the constants {b, e, cst} of every cluster (direction_far, niw_sweep.hip)
        const float *brk_aref;     // D = 128, 256: per position of the visiting order the bracket's lower end of a_k0 (launch_niw_bracket_big)
    };
    uint32_t *need;           // [waves][2] (pinned host memory, may be null): [0] = (candidates this wave's tiles kept behind the 4-row tests, saturating) << 16 | tiles
                              // (15 bits), bit 15: counted in FRONT of the tail-pair tests (direction screen first): an upper bound;
                              // [1] (written by the DIR kernel only) = (candidates its direction screens removed) << 16 | candidates they were given
    union {
        unsigned long long *dbg;   // diagnostic builds (DPMM_STAMPS): per-wave phase cycle sums
        uint8_t *cert_points;      // product build, lean launch only: a byte per point of the shard, set for the points of the tiles the norm certificate
                                   // settled (dpmm_debug_norm_cert_points; null unless that call switched the record on)
    };
    int queue_rounds;         // D <= 64 kernel: rounds of tiles handed out through the queue at the end of the launch (-1: automatic)
    int prio;                 // 1: s_setprio -- low while the wave streams MFMAs, high in its scalar / VALU phases (DPMM_OPT_WAVE_PRIO)
    unsigned long long *work; // [4] tile queue head of the LDS-staged kernel, [8 + 16 q], q < 8: the eight queue heads of the D <= 64 kernel (one 128-byte
                              // line each), all cleared before the launch; [DPMM_WORK_SLOTS + DPMM_WORK_PER_WAVE w ..]: executed-work counters of
                              // wave w of this launch (wave tiles, full evaluations, 16-row screens, tail-screened cluster pairs, reference brackets), plain
                              // stores at kernel end, summed by the reader; may be null
};
// The argument block's size decides how the compiler lays out its scalars (a field of its own for one flag bit cost the common kernel 32 spilled
// registers), so the layout is pinned: a change that moves any of this re-lays every sweep kernel's scalars and has to be measured as a kernel change.
static_assert(sizeof(NiwSweepArgs) == 256, "NiwSweepArgs: frozen size");
static_assert(offsetof(NiwSweepArgs, tdf) == 72 && offsetof(NiwSweepArgs, tile_list) == 72, "NiwSweepArgs: frozen layout");
static_assert(offsetof(NiwSweepArgs, ball) == 164 && offsetof(NiwSweepArgs, bf16scr) == 168, "NiwSweepArgs: frozen layout");
static_assert(offsetof(NiwSweepArgs, mdist) == 184 && offsetof(NiwSweepArgs, list_len) == 184, "NiwSweepArgs: frozen layout");
static_assert(offsetof(NiwSweepArgs, sp_frag) == 208 && offsetof(NiwSweepArgs, brk_flag) == 208, "NiwSweepArgs: frozen layout");
static_assert(offsetof(NiwSweepArgs, sp_cons) == 216 && offsetof(NiwSweepArgs, brk_aref) == 216, "NiwSweepArgs: frozen layout");
static_assert(offsetof(NiwSweepArgs, dbg) == 232 && offsetof(NiwSweepArgs, cert_points) == 232, "NiwSweepArgs: frozen layout");
static_assert(offsetof(NiwSweepArgs, work) == 248, "NiwSweepArgs: frozen layout");

// What a caller of launch_niw_sweep asks for beyond the block (host side only, D in 33..64): the label-storing instantiations -- labels drawn and stored,
// niw_sub_kernel draws the sub-labels -- for every tile or for the spans of tile_list; the launcher writes NiwSweepArgs::tile_list / list_len itself.
struct NiwLabelStore {
    bool store_labels = false;
    const uint32_t *tile_list = nullptr;   // device: [0] = count, [1 ..] = spans (null: all tiles)
    uint32_t *list_len = nullptr;          // pinned host word (nullable), written only when a list is walked
};

int niw_tile_points(int NB);
int niw_occupancy(int NB);  // resident 256-thread workgroups per CU the sweep kernel is built for
hipError_t launch_niw_sweep(int NB, const NiwSweepArgs &a, int grid, hipStream_t s, const NiwLabelStore &ls = {});
hipError_t launch_niw_refb_debug(const NiwSweepArgs &a, int k, float c_override, float *qhi_out, float *q_out, hipStream_t s);   // needs X, ldx, n, K, Rp, mup, tail
hipError_t launch_niw_screen_prep(const float *R, const float *mu, int D, int K, float *lam, float *dist, const int32_t *slot, hipStream_t s);
hipError_t launch_niw_pack(const float *R, const float *mu, float *Rp, float *mup, int D, int NB, int nmat, float *tail, const float *cst,
                           const int32_t *slot, float *cst_out, unsigned long long *work, hipStream_t s);
// Tables of the direction screen from the sweep's own images (Rp, mup, cst of the K cluster-level distributions; D in 33..64, K <= SP_MAXK):
// frag [K][SP_FRAG_WORDS], cons [K][SP_CONS_FLOATS]
constexpr int SP_MAXK = 64, SP_FRAG_WORDS = 4 * 2 * 256, SP_CONS_FLOATS = 3 * 64;
// The launch-independent part of "this launch is a steady-state one" (the FAST instantiations; launch_direct adds NB >= 2 and the LDS budget, which every
// K <= SP_MAXK meets at D in 33..64), and THE condition of the direction-screen instantiations (DIR) on top of it: the tables are there, the bf16 screens
// are on and K fits.  launch_direct, launch_niw_lean (which asks K >= 3 more) and run_sweep's record of "the DIR kernel wrote its yield words" all ask here.
inline bool niw_steady_launch(const NiwSweepArgs &a, bool store_labels) {
    return a.screen_margin > 0.f && (store_labels || !a.tdf) && !a.scratch_by_tile && !a.labels_only && a.K > 1 && a.lam == nullptr && a.tail != nullptr && !a.final_argmax;
}
inline bool niw_dir_screen(const NiwSweepArgs &a) { return a.sp_frag && a.sp_cons && a.bf16scr && a.K <= SP_MAXK; }
// bf16 images of the K cluster-level factors for the reference bracket of the LDS-staged kernels (NB = 8, 16), from the Float32 fragment
// image: out [K][niw_refb_big_words(NB)]  (launch_niw_bracket_big reads it; the sweep sees that launch's output as brk_flag / brk_aref)
inline size_t niw_refb_big_words(int NB) { size_t c = 0; for (int bi = 0; bi < NB; ++bi) c += NB / 2 - bi / 2; return c * 256; }
hipError_t launch_niw_refb_big(const float *Rp, int NB, int K, uint32_t *out, hipStream_t s);
// the bracket itself, in front of the sweep launch (same NiwSweepArgs: X, order, bins, mup, cst): tile_flag [ceil(n / 128)], aref [128 ceil(n / 128)]
hipError_t launch_niw_bracket_big(int NB, const NiwSweepArgs &a, const uint32_t *refb, uint32_t *tile_flag, float *aref, hipStream_t s);
// ---- niw_lean.hip: the bf16 three-plane evaluation of the sub-cluster quadratic forms (NB = 4)
// images [3K][B3_WORDS] and offset vectors [3K][B3_DVEC] of the 2K sub-cluster factors from the Float32 fragment image, written behind the bracket's images in `tail`
hipError_t launch_niw_b3_pack(const float *Rp, const float *mup, int K, float *tail, int what, hipStream_t s);      // what bit 0: images + offsets; bit 1: the pair-ball table (2 <= K <= PB_MAXK) behind them; bit 2: with the tight sn2 block (else sn2 = sn)
// the pair-ball table behind the offsets (round 6; K <= PB_MAXK): pd [K][K] -- pd[k K + j] = a certified LOWER bound of |R_j (mu_k - mu_j)|, the distance of
// cluster k's mean from cluster j's in j's own metric -- and sn [K], certified UPPER bounds of the spectral norms |R_j|_2 (niw_pair_ball_kernel, niw_lean.hip)
// and sn2 [K] behind them: tighter certified upper bounds of the same norms (power bound, PB_NORM_SQUARINGS squarings of R' R in Float64; sn2 <= sn) for the lean kernel's norm certificate
constexpr int PB_MAXK = 256;
#ifndef DPMM_PB_NORM_SQUARINGS
#define DPMM_PB_NORM_SQUARINGS 3
#endif
constexpr int PB_NORM_SQUARINGS = DPMM_PB_NORM_SQUARINGS;      // (hand-over launch 17.2 us without the block; DESIGN 10 has the cost and the hit rate for 1, 2, 3)
inline size_t niw_pair_ball_floats(size_t K) { return K <= (size_t)PB_MAXK ? K * K + 2 * K : 0; }
inline size_t niw_pair_ball_offset(size_t K) { return 32 * ((K + 1) >> 1) + 16 * K + (size_t)REFB_WORDS * K + 3 * K * (size_t)B3_WORDS + 3 * K * (size_t)B3_DVEC; }      // floats from `tail` (= b3_offsets(tail, K) + 3 K B3_DVEC, niw_b3.h)
inline size_t niw_tail_floats(size_t cap) {      // pair records | ball records | bracket images | b3 images | b3 offsets | pair-ball table
    return 16 * (cap + 2) + 16 * cap + (size_t)REFB_WORDS * cap + 3 * cap * (size_t)B3_WORDS + 3 * cap * (size_t)B3_DVEC + niw_pair_ball_floats(cap < (size_t)PB_MAXK ? cap : (size_t)PB_MAXK);
}
// out [2K][n]: both sub-cluster values of every point under every cluster (needs X, ldx, n, K, mup, cst, tail)
hipError_t launch_niw_b3_debug(const NiwSweepArgs &a, float *out, hipStream_t s);
// the sub-label phase alone for the wave tiles of `list` (list[0] = count, list[1 ..] = tile indices; null: all tiles); labels are read from bins
hipError_t launch_niw_sub(const NiwSweepArgs &a, const uint32_t *list, uint32_t *count_out, int grid, hipStream_t s);      // count_out (pinned, nullable): receives list[0]
// whole tiles where bracket + ball + tail screens settle them (every point had label k0, nothing else can compete): labels AND sub-labels; every
// other tile is appended to list ([0] = count, cleared by the caller; [1 ..] = wave-tile indices) and left untouched.  need2 [4 grid] (nullable, pinned): tiles settled per wave
constexpr int NIW_LEAN_MAX_BINS = 256;      // bins of the sort the lean kernel can align its tiles to (beyond: tiles of 64 consecutive positions)
// bin_start [nbins + 1] (nullable): the offsets of the sort that wrote a.order -- tiles never cross a bin.  The list holds (position, count) pairs:
// 1 + 2 * (ceil(n / 64) + nbins) words at most.
hipError_t launch_niw_lean(const NiwSweepArgs &a, uint32_t *list, uint32_t *need2, uint32_t *other_list, const int32_t *bin_start, int nbins, uint32_t *need3, int grid, hipStream_t s);      // list[0] must be 0; other_list[0] is cleared for the next launch
hipError_t launch_niw_direction(const float *Rp, const float *mup, const float *cst, int D, int K, uint32_t *frag, float *cons, hipStream_t s);

struct MultSweepArgs {
    const float *X;
    int64_t ldx;
    int64_t n;
    int64_t first_index;
    int D;
    int K;
    const float *logp;   // packed fragment image Lp[ceil(3K/16)][ceil(ldx/16)][64][4]
    const float *cst;    // [3K]: 3k: log w_k ; 3k+1+s: log lr_w[k][s]
    float *scratch;
    int64_t scratch_stride;
    int scratch_by_tile;
    int labels_only;
    int32_t *bins;
    uint64_t seed;
    uint32_t epoch;
    int final_argmax;
    // u8 kernel: previous labels are valid (row-block selection), bin-sorted visiting order of the last statistics pass (nullable)
    int use_prev;
    const int32_t *order;
    const int32_t *order_total;
};
hipError_t launch_mult_sweep(const MultSweepArgs &a, int grid, hipStream_t s);
hipError_t launch_mult_pack(const float *logp, float *Lp, int rows, int64_t ldx, hipStream_t s);
int mult_tile_points();
// bf16 path (count data): exactness check of X, 3-plane bf16 split of the log-probabilities, sweep
hipError_t launch_bf16_exact_check(const float *X, int64_t nwords, int *d_flag, hipStream_t s);
size_t mult_pack_bf16_words(int rows, int64_t ldx);
hipError_t launch_mult_pack_bf16(const float *logp, uint32_t *Lp16, int rows, int64_t ldx, hipStream_t s);
hipError_t launch_mult_sweep_bf16(const MultSweepArgs &a, const uint32_t *Lp16, int grid, hipStream_t s);
// u8 path (integer data in [0, 255]): byte copy of the points, parameter planes in the matching feature order, sweep, statistics
hipError_t launch_u8_convert(const float *X, int64_t ldx, int D, int64_t n, uint8_t *X8, int64_t ld8, int *d_flag, hipStream_t s);
size_t mult_pack_u8_words(int rows, int64_t ld8);
hipError_t launch_mult_pack_u8(const float *logp, uint32_t *Lp8, int rows, int64_t ldx, int64_t ld8, hipStream_t s);
hipError_t launch_mult_sweep_u8(const MultSweepArgs &a, const uint8_t *X8, int64_t ld8, const uint32_t *Lp8, int grid, hipStream_t s);

// ---- points stored as compressed sparse columns (mult_sparse.hip): cp [n + 1] offsets, ri [nnz] feature indices (strictly increasing inside
// a column), val [nnz] values (none zero); T [D][3K] the transposed parameter image: columns [0, K) = rows 3k, column K + 2k + s = row 3k + 1 + s
struct MultSparse {
    const int64_t *cp;
    const uint16_t *ri;
    const float *val;
    const float *T;
    unsigned *ticket;    // [1] tile counter of the sweep kernel (cleared by its launcher)
};
hipError_t launch_csc_check(const int64_t *cp, const int64_t *rv, const float *nz, int64_t n, int64_t total, int D, int base, int32_t *cnt,
                            unsigned long long *bad, hipStream_t s);
hipError_t launch_csc_compact(const int64_t *cp, const int64_t *rv, const float *nz, int64_t n, int base, const int64_t *cp_out, uint16_t *ri, float *val,
                              hipStream_t s);
hipError_t launch_mult_pack_sparse(const float *logp, float *T, int K, int D, int64_t ldx, hipStream_t s);
hipError_t launch_mult_sweep_sparse(const MultSweepArgs &a, const MultSparse &sp, int grid, hipStream_t s);      // a.X, a.logp, a.order are not read
struct StatsArgs;
hipError_t launch_mult_stats_sparse(const StatsArgs &a, const MultSparse &sp, hipStream_t s);                    // a.X is not read
hipError_t launch_mult_reduce(const StatsArgs &a, hipStream_t s);

// ---- label bookkeeping (labels.hip)
// dst/src: device or pinned-host pointers, 4-byte aligned; bytes rounded up to a multiple of 4
hipError_t launch_smart_project(const int32_t *bins, const float *X, int64_t ldx, int64_t n, int D, int k, const double *v, const double *mu,
                                double *proj, double *vals, unsigned long long *counter, hipStream_t s);
hipError_t launch_smart_kmeans(const int32_t *bins, const double *proj, int64_t n, int k, double m_lo, double m_hi, double *partial, double *out,
                               hipStream_t s);
hipError_t launch_smart_assign(int32_t *bins, const double *proj, int64_t n, int k, double m_lo, double m_hi, hipStream_t s);
int smart_groups();
hipError_t launch_predict_finish(const float *table, int64_t stride, int rstep, int64_t n, int K, int64_t *labels, float *probs, hipStream_t s);
// ---- scoring (score.hip; include/dpmm_hip_score.h): the fused finish over one slab of the table, n points from table column 0; every
// output pointer is that of the slab's first point and may be null (top_idx / top_prob: [n][m], m <= 16; probs: [n][K])
struct ScoreArgs {
    const float *table;
    int64_t stride;      // floats between two rows of the table
    int rstep;           // cluster k is row k * rstep
    int64_t n;
    int K;
    int64_t *labels;
    float *logdens;
    int m;
    int64_t *top_idx;
    float *top_prob;
    float *probs;
};
hipError_t launch_score_finish(const ScoreArgs &a, hipStream_t s);
// ---- exemplars (rank.hip; include/dpmm_hip_rank.h): one chunk of at most `cap` points of a slab of the table, from table column 0, against
// the running lists; then the lists decoded for the caller
constexpr int RANK_SLOTS = 64;            // keys of a running list (DPMM_RANK_MAX_M), one per lane of the merging wave
constexpr int RANK_REPL = 8;              // replicas of the counters [K + 1] (count | skipped); a workgroup adds to replica blockIdx % 8
constexpr int64_t RANK_CHUNK = 262144;    // points per filter launch at most = entries of a candidate buffer
struct RankArgs {
    const float *table;
    int64_t stride;      // floats between two rows of the table
    int rstep;           // cluster k is row k * rstep
    int64_t n;           // points of this chunk, n <= cap
    int K;
    int64_t index0;      // global index of the chunk's first point; index0 + n <= 2^32
    int m, which;        // which bit 0: typical list, bit 1: fringe list
    unsigned long long *keys;       // [2][K][RANK_SLOTS] the running lists, typical | fringe, largest key first, 0 = empty
    unsigned long long *count;      // [RANK_REPL][K + 1]
    unsigned long long *cand_key;   // [2][cap]
    uint16_t *cand_k;               // [2][cap] 0-based cluster of the candidate
    unsigned *cand_n;               // [2][2] candidates of (parity, list); the launch clears those of parity ^ 1
    int64_t cap;
    int parity;
};
struct RankOut { int64_t *typ_idx; float *typ_score; int64_t *fringe_idx; float *fringe_score; int64_t *count; int64_t *skipped; };      // = dpmm_rank_out
hipError_t launch_rank_chunk(const RankArgs &a, hipStream_t s);
hipError_t launch_rank_read(const unsigned long long *keys, const unsigned long long *count, int K, int m, int which, const RankOut &o, hipStream_t s);
// ---- cluster overlap (overlap.hip; include/dpmm_hip_overlap.h): one range of the score table, n points from table column 0, added to the
// ctx's accumulators
constexpr int OVERLAP_PARTIAL_BLOCKS = 512;      // DPMM_OVERLAP_PARTIAL_BLOCKS: 64 x 64 blocks of chunk partials at most
struct OverlapArgs {
    const float *table;
    int64_t stride;      // floats between two rows of the table
    int rstep;           // cluster k is row k * rstep
    int64_t n;           // points of the range that are accumulated
    int K;
    int nb;              // row blocks of 64 clusters, (K + 63) / 64
    int nchunk;          // chunks of the range (overlap_chunks)
    int64_t chunk;       // points per chunk, a multiple of 64
    float2 *ms;                     // [n] (M, S) of the point; S = 0: it takes no part
    unsigned long long *count;      // [RANK_REPL][K + 1] count | skipped
    double *part;                   // [nchunk][nb (nb + 1) / 2][64][64] partial blocks of the lower block triangle
    double *mpart;                  // [nchunk][nb * 64] partial masses
    double *acc;                    // [K][K] overlap | [K] mass
};
void overlap_chunks(int64_t n, int K, int *nchunk, int64_t *chunk);
hipError_t launch_overlap_range(const OverlapArgs &a, hipStream_t s);
// ---- per-cluster batch statistics (batchstats.hip; include/dpmm_hip_batchstats.h): one range of the score table, n points from table
// column 0 and from X, added to the ctx's accumulators
constexpr int BATCHSTATS_PARTIAL_BLOCKS = 2048;  // DPMM_BATCHSTATS_PARTIAL_BLOCKS: 64 x 64 blocks of chunk partials at most
constexpr int BATCHSTATS_COUNTERS = 3;           // behind count[K]: skipped | held out | incomplete
struct BatchStatsArgs {
    const float *table;
    int64_t stride;      // floats between two rows of the table
    int rstep;           // cluster k is row k * rstep
    int64_t n;           // points of the range that are accumulated, below 2^31
    int K, D;
    const float *X;      // [n][ldx], the range's first point
    int64_t ldx;
    int soft;            // 0: w_ik = [label_i == k + 1], 1: w_ik = p_ik
    int use_floor;       // points with logdens < min_logdens are held out
    float min_logdens;
    int use_tail;        // complete points with tail[i] < min_tail are held out (include/dpmm_hip_typicality.h)
    float min_tail;
    const float *tail;   // [n] the range's tails as launch_typicality_range wrote them (NaN: skipped or incomplete); read only if use_tail
    int nb;              // blocks of 64 features, (D + 63) / 64
    int kgroup;          // clusters per contraction launch (batchstats_chunks)
    int nchunk;          // chunks of the range (batchstats_chunks)
    int64_t chunk;       // points per chunk, a multiple of 64
    int k0, kcount;      // the clusters of one contraction / reduce launch (set by launch_batchstats_range)
    float2 *ms;                     // [n] soft: (M, S) of the point; hard: (label, 1); y = 0: it takes no part
    unsigned long long *count;      // [RANK_REPL][K + BATCHSTATS_COUNTERS]
    double *part;                   // [nchunk][kcount][nb (nb + 1) / 2][64][64] partial blocks of the lower block triangle
    double *spart;                  // [nchunk][kcount][nb * 64] partial sums
    double *npart;                  // [nchunk][kcount] partial weights
    double *acc;                    // [K] N | [K][D] sums | [K][D][D] S
};
void batchstats_chunks(int64_t n, int K, int D, int *kgroup, int *nchunk, int64_t *chunk);
hipError_t launch_batchstats_range(const BatchStatsArgs &a, hipStream_t s);
// ---- held-out points (holdout.hip; include/dpmm_hip_holdout.h): one range of the score table, n points from table column 0 and from X; the
// points the rule of BatchStatsArgs holds out are appended to the caller's buffers in increasing index
constexpr int HOLDOUT_THREADS = 256;             // points per workgroup of the class and gather passes
constexpr int HOLDOUT_STATE = 4;                 // running totals: held out | skipped | incomplete | taking part
inline int64_t holdout_groups(int64_t n) { return (n + HOLDOUT_THREADS - 1) / HOLDOUT_THREADS; }
// the compaction of a range, whatever the prior: all that the scan and the row gather see
struct HoldoutCompact {
    int64_t n;           // points of the range that are classified, below 2^31
    int64_t index0;      // global index of the range's first point
    unsigned long long *ballot;     // [4 * holdout_groups(n)] bit l of word j: point 64 j + l is held out
    unsigned *wgcount;              // [holdout_groups(n)][HOLDOUT_STATE] the classes of the workgroup's points, counted
    int64_t *wgoff;                 // [holdout_groups(n)] slot of the workgroup's first held-out point
    unsigned long long *state;      // [HOLDOUT_STATE] running totals: read, then advanced, by the scan (count data: [COUNTHOLDOUT_STATE])
    float *dst_points;              // [cap][D] (rows: NIW and the dense count stores)
    int64_t *dst_index;             // [cap]
    int64_t cap;
};
struct HoldoutArgs : HoldoutCompact {
    const float *table;
    int64_t stride;      // floats between two rows of the table
    int rstep;           // cluster k is row k * rstep
    int K, D;
    const float *X;      // [n][ldx], the range's first point
    int64_t ldx;
    int use_floor;       // as BatchStatsArgs
    float min_logdens;
    int use_tail;
    float min_tail;
    const float *tail;   // [n], read only if use_tail
};
hipError_t launch_holdout_range(const HoldoutArgs &a, hipStream_t s);
// ---- per-cluster count statistics of the Multinomial prior (countstats.hip; include/dpmm_hip_countstats.h): one range of the score table,
// n points from table column 0 and from whichever point store is live, added to the ctx's accumulators
constexpr int64_t COUNTSTATS_PARTIAL_BYTES = (int64_t)64 << 20;      // DPMM_COUNTSTATS_PARTIAL_BYTES: the chunk partials at most
constexpr int COUNTSTATS_F32 = 0, COUNTSTATS_U8 = 1, COUNTSTATS_SPARSE = 2;
struct CountStatsArgs {
    const float *table;
    int64_t stride;      // floats between two rows of the table
    int rstep;           // cluster k is row k * rstep
    int64_t n;           // points of the range that are accumulated, below 2^31
    int K, D;
    int store;           // COUNTSTATS_F32: X [n][ldx]; _U8: X8 [n][ld8]; _SPARSE: cp / ri / val (cp at the range's first point)
    const float *X;
    int64_t ldx;
    const uint8_t *X8;
    int64_t ld8;
    const int64_t *cp;
    const uint16_t *ri;
    const float *val;
    int soft;            // 0: w_ik = [label_i == k + 1], 1: w_ik = p_ik
    int use_floor;       // points with logdens < min_logdens are held out
    float min_logdens;
    int use_pc;          // complete points with t_i > 0 and (double)logdens < (double)min_pc * t_i are held out too
    float min_pc;
    const double *tot;   // [n] t_i as launch_countstats_totals wrote them, read only if use_pc
    int kgroup;          // clusters per contraction launch (countstats_chunks): a multiple of 16 for the dense stores
    int nchunk;          // chunks of the range (countstats_chunks)
    int64_t chunk;       // points per chunk, a multiple of 64
    int64_t dp;          // doubles per cluster row of the partials, >= D (countstats_chunks)
    int k0, kcount, krows;   // the clusters of one contraction / reduce launch and the rows their partials have (set by launch_countstats_range)
    float2 *ms;                     // [n] soft: (M, S) of the point; hard: (label, 1); y = 0: it takes no part
    unsigned long long *count;      // [RANK_REPL][K + BATCHSTATS_COUNTERS]
    double *part;                   // [nchunk][krows][dp] partial sums
    double *npart;                  // [nchunk][krows] partial weights
    double *acc;                    // [K] N | [K][D] sums
};
void countstats_chunks(int64_t n, int K, int D, int sparse, int *kgroup, int *nchunk, int64_t *chunk, int64_t *dp);
hipError_t launch_countstats_range(const CountStatsArgs &a, hipStream_t s);
// t_i, the Float64 total of the values of every point of a range, for the floor per count (countstats.hip): one wave per point
struct CountTotalsArgs {
    int64_t n;           // points of the range, below 2^31
    int D;
    int store;           // as CountStatsArgs, the pointers at the range's first point (cp) / the whole entry arrays (val)
    const float *X;
    int64_t ldx;
    const uint8_t *X8;
    int64_t ld8;
    const int64_t *cp;
    const float *val;
    double *tot;         // [n]
};
hipError_t launch_countstats_totals(const CountTotalsArgs &a, hipStream_t s);
// ---- held-out points of count data (holdout.hip; include/dpmm_hip_countholdout.h): one range of the score table, n points from table
// column 0 and from whichever point store is live; the points the rule of countstats_device.h holds out are appended to the caller's buffers
// in increasing index -- rows of Float32 for the dense stores, compressed sparse columns for the sparse one
constexpr int COUNTHOLDOUT_STATE = 8;            // running totals: held out | skipped | incomplete | taking part | held-out entries | stored | stored entries | unused
constexpr unsigned long long COUNTHOLDOUT_UNSET = ~0ull;      // stored / stored entries while every held-out point so far has fitted
struct CountHoldoutArgs : HoldoutCompact {      // state: [5], [6] are written by the one boundary workgroup of the sparse gather
    const float *table;
    int64_t stride;      // floats between two rows of the table
    int rstep;           // cluster k is row k * rstep
    int K, D;
    int store;           // as CountStatsArgs
    const float *X;
    int64_t ldx;
    const uint8_t *X8;
    int64_t ld8;
    const int64_t *cp;
    const uint16_t *ri;
    const float *val;
    int use_floor;       // as CountStatsArgs
    float min_logdens;
    int use_pc;
    float min_pc;
    const double *tot;
    unsigned long long *wgent;      // [holdout_groups(n)] stored entries of the workgroup's held-out points (sparse store; else 0)
    int64_t *wgeoff;                // [holdout_groups(n)] entry offset of the workgroup's first held-out point
    int64_t *dst_colptr;            // sparse store: [cap + 1]
    int32_t *dst_rowval;            // [entry_cap]
    float *dst_val;                 // [entry_cap]
    int64_t entry_cap;
};
hipError_t launch_countholdout_range(const CountHoldoutArgs &a, hipStream_t s);
// ---- missing features (missing.hip; include/dpmm_hip_missing.h): one range of the score table, n points from table column 0 and from X
constexpr int MISS_MAX = 16;              // DPMM_SCORE_MAX_MISSING
constexpr int MISS_CST = MISS_MAX + 2;    // doubles per cluster in MissArgs::cst
inline int miss_pitch(int D) { return 64 * ((D + 63) / 64); }
struct MissArgs {
    float *table;                // entry (k, i) at table[k * stride + i]; the patch kernel rewrites the listed points' entries
    int64_t stride;
    int64_t n;
    int K, D;
    const float *X;              // [n][ldx], the range's first point
    int64_t ldx;
    const float *Rt;             // [K][D][miss_pitch(D)]: Rt[k][j][i] = R_k[i][j], zero below the diagonal (i > j) and in the pad (i >= D)
    const float *mu;             // cluster k's mean: mu + k * mu_step
    int64_t mu_step;
    const double *cst;           // [K][MISS_CST]: [0] = df, [r], 1 <= r <= MISS_MAX: lgamma((df + D - r) / 2) - lgamma(df / 2) - (D - r) / 2 log(df pi) - logdet / 2 + log w
    uint32_t *list;              // [n] positions of the range's points with 1 .. min(MISS_MAX, D - 1) NaN features, in no particular order
    unsigned long long *cnt;     // [0] entries of list (cleared per range), [1] marginalised, [2] over-the-cap points (cleared per call)
    float *out;                  // impute: [n][ld_out] rows the points were copied to; the NaN words of listed points are rewritten
    int64_t ld_out;
};
hipError_t launch_miss_transpose(const float *Rpk, int64_t step, float *Rt, int K, int D, hipStream_t s);      // Rpk: packed upper triangles, cluster k at Rpk + k * step
hipError_t launch_miss_list(const MissArgs &a, hipStream_t s);
hipError_t launch_miss_patch(const MissArgs &a, bool impute, int max_grid, hipStream_t s);
// ---- mixture regression (regress.hip; include/dpmm_hip_regress.h): one range of the score table, n points from table column 0 and from X
constexpr int REGRESS_MAX_TARGETS = 256;  // DPMM_REGRESS_MAX_TARGETS
inline int regress_pitch(int Dt) { return 32 * ((Dt + 31) / 32); }
// what the kernels of regress.hip and regress_draw.hip share (regress_device.h)
struct RegressTile {
    const float *table;          // entry (k, i) at table[k * stride + i] (NIW: one row per cluster)
    int64_t stride;
    int64_t n;
    int K, D;                    // D: the given features, the ctx's dimension
    int Dt, Tp;                  // targets; Tp = regress_pitch(Dt)
    const float *X;              // [n][ldx], the range's first point
    int64_t ldx;
    const float *c;              // [K][Tp], zero in the pad
    const double *hd;            // [K][2]: h_k, df_k
    int64_t *labels;             // [n] or null
    unsigned *skip;              // [ceil(n / 32)] points of tile j that take no part, ADDED to word j
};
// the shapes the launchers of regress.hip and regress_draw.hip refuse; ld: floats between two rows of its outputs
inline bool regress_tile_ok(const RegressTile &t, int64_t ld) {
    return t.K >= 1 && t.D >= 1 && t.Dt >= 1 && t.Tp % 32 == 0 && t.Tp >= t.Dt && ld >= t.Dt && !(((t.n + 31) / 32) >> 31);
}
struct RegressArgs {
    RegressTile t;
    const float *Bt;             // [K][D][Tp]: Bt[k][e][d] = B_k[d][e], zero in the pad (d >= Dt)
    const float *V;              // [K][Tp], zero in the pad
    float *mean, *std;           // [n][ld] rows of the range's points; std null: not asked for
    int64_t ld;
};
hipError_t launch_regress_range(const RegressArgs &a, hipStream_t s);
// ---- top-m next-count probabilities (recommend.hip; include/dpmm_hip_recommend.h): one range of the score table, n points from table
// column 0 and from whichever count store is live
constexpr int RECOMMEND_MAX_TOP = 16;     // DPMM_RECOMMEND_MAX_TOP
inline int64_t recommend_pitch(int D) { return 32 * (((int64_t)D + 31) / 32); }
struct RecommendArgs {
    const float *table;
    int64_t stride;      // floats between two rows of the table
    int rstep;           // cluster k is row k * rstep
    int64_t n;
    int K, Kp;           // Kp = K rounded up to even
    int D;
    int64_t Dp;          // recommend_pitch(D)
    int store;           // as CountStatsArgs, the pointers at the range's first point (X, X8, cp) / the whole entry arrays (ri, val)
    const float *X;
    int64_t ldx;
    const uint8_t *X8;
    int64_t ld8;
    const int64_t *cp;
    const uint16_t *ri;
    const float *val;
    const float *theta;  // [Kp][Dp], zero in the pad
    int m, exclude;      // 1 <= m <= min(D, RECOMMEND_MAX_TOP); exclude: the features a point has seen are no candidates
    int32_t *features;   // [n][ld] rows of the range's points, 0-based, -1 behind the candidates
    float *prob;         // [n][ld], NaN behind the candidates
    int64_t ld;
    int64_t *labels;     // [n] or null
    unsigned *skip;      // [ceil(n / 32)] points of tile j that take no part, ADDED to word j
};
hipError_t launch_recommend_range(const RecommendArgs &a, hipStream_t s);
// ---- top-m surprising features of a count point (count_explain.hip; include/dpmm_hip_count_explain.h): one range of the score table, n
// points from table column 0 and from whichever count store is live
constexpr int COUNT_EXPLAIN_MAX_TOP = 16; // DPMM_COUNT_EXPLAIN_MAX_TOP
constexpr int COUNT_EXPLAIN_TILE = 32;    // points of a wave: one counter word each in `skip` and `incomplete`
enum { COUNT_EXPLAIN_BOTH = 0, COUNT_EXPLAIN_OVER = 1, COUNT_EXPLAIN_UNDER = 2 };      // DPMM_COUNT_EXPLAIN_*
struct CountExplainArgs {
    const float *table;
    int64_t stride;      // floats between two rows of the table
    int rstep;           // cluster k is row k * rstep
    int64_t n;
    int K, D;
    int store;           // as CountStatsArgs, the pointers at the range's first point (X, X8, cp) / the whole entry arrays (ri, val)
    const float *X;
    int64_t ldx;
    const uint8_t *X8;
    int64_t ld8;
    const int64_t *cp;
    const uint16_t *ri;
    const float *val;
    const double *lth;   // [K][D] log theta
    const double *l1m;   // [K][D] log1p(-theta)
    const int32_t *order;// [K][D] the features of cluster k with l1m non-decreasing (theta non-increasing), ties to the lower index
    int top, side;       // 1 <= top <= min(D, COUNT_EXPLAIN_MAX_TOP); side: COUNT_EXPLAIN_*
    int32_t *features;   // [n][ld] rows of the range's points, 0-based, -1 behind the candidates
    float *count;        // [n][ld] each, NaN behind the candidates
    float *expected;
    float *residual;
    float *feature_tail;
    int64_t ld;
    int64_t *labels;     // [n] or null
    double *total;       // [n] or null: t_i, NaN for a skipped point
    double *tot;         // [n] the ctx's own copy of total, and the 0-based labels: what the tail kernel reads
    int32_t *lab;
    unsigned *skip;      // [ceil(n / COUNT_EXPLAIN_TILE)] skipped points of tile j, ADDED to word j
    unsigned *incomplete;// ... and incomplete ones
};
hipError_t launch_count_explain_range(const CountExplainArgs &a, hipStream_t s);
// ---- draws of the targets (regress_draw.hip; include/dpmm_hip_regress_draw.h): one range of the score table, n points from table column 0
// and from X, the draws draw0 .. draw0 + ndraws - 1 of each
constexpr int64_t REGRESS_DRAW_MAX = 67108864;      // DPMM_REGRESS_MAX_DRAWS
struct RegressDrawArgs {
    RegressTile t;               // labels: not written; skip null: not counted by this launch
    const float *Bw;             // [K][D + Dt][Tp]: rows [0, D) of cluster k are RegressArgs::Bt[k]; row D + a is W_k[.][a] (Bw[k][D + a][d] = W_k[d][a]),
                                 // zero below the diagonal of W (a < d) and in the pad (d >= Dt)
    float *out;                  // element (jd, i, f) at out[jd * draw_stride + i * ld + f], f < min(ld, draw_stride); columns [Dt, ..) are written as 0
    int64_t ld, draw_stride;
    int32_t *comp;               // null, or element (jd, i) at comp[jd * comp_stride + i]
    int64_t comp_stride;
    uint64_t seed;
    int64_t i0;                  // global index of the range's first point
    int64_t draw0;
    int ndraws;
    int32_t *kc;                 // scratch [ndraws][n]: the drawn cluster (-1: the point's row of the table takes no part) and
    float *sc;                   // the scale s of every (draw, point), written by the first kernel of the launch and read by the second
};
hipError_t launch_regress_draw_range(const RegressDrawArgs &a, hipStream_t s);
// ---- conditional CDF and quantiles of the targets (regress_cdf.hip; include/dpmm_hip_regress_cdf.h): one range of the score table, n points
// from table column 0 and from X; table .. hd, labels and skip as RegressTile and RegressArgs.  The two structs keep these fields flat and in this
// order: the kernels of regress_cdf.hip sit at the register limit, and are compiled exactly as they were
constexpr int REGRESS_MAX_LEVELS = 16;    // DPMM_REGRESS_MAX_LEVELS
struct RegressCdfArgs {
    const float *table;
    int64_t stride;
    int64_t n;
    int K, D;
    int Dt, Tp;
    const float *X;
    int64_t ldx;
    const float *Bt;
    const float *c, *V;
    const double *hd;
    const float *y;              // [n][ldy] the observed targets of the range's points
    int64_t ldy;
    float *cdf, *sf;             // [n][ld]; sf null: not asked for
    int64_t ld;
    int64_t *labels;
    unsigned *skip;
};
hipError_t launch_regress_cdf_range(const RegressCdfArgs &a, hipStream_t s);
struct RegressQuantileArgs {
    const float *table;
    int64_t stride;
    int64_t n;
    int K, D;
    int Dt, Tp;
    const float *X;
    int64_t ldx;
    const float *Bt;
    const float *c, *V;
    const double *hd;
    const double *levels;        // [L], increasing
    const double *z;             // [K][L]: the level's quantile of t_{df_k + D}
    const double *lc;            // [K]: log of the density of t_{df_k + D} at 0
    int L;
    float *out;                  // element (i, q, d) at out[(i * L + q) * ld + d]; columns [Dt, ld) are written as 0
    int64_t ld;
    int64_t *labels;
    unsigned *skip;
};
hipError_t launch_regress_quantile_range(const RegressQuantileArgs &a, hipStream_t s);
// ---- calibrated outlier scores (typicality.hip; include/dpmm_hip_typicality.h): one range of the score table, n points from table column 0:
// the label and the class of every point, q = |R_k (x - m_k)|^2 for its own cluster k in Float32, the tail of q in Float64
struct TypicalityArgs {
    const float *table;          // entry (k, i) at table[k * stride + i] (NIW: one row per cluster)
    int64_t stride;
    int64_t n;
    int K, D;
    const float *X;              // [n][ldx], the range's first point
    int64_t ldx;
    const float *Rt;             // as MissArgs::Rt
    const float *mu;             // cluster k's mean: mu + k * mu_step
    int64_t mu_step;
    const double *cst;           // as MissArgs::cst: [k * MISS_CST] = df_k, the Float32 value widened
    int32_t *cls;                // [n] scratch: the 0-based cluster of the point, -1 for a skipped one
    int64_t *labels;             // [n] or null
    float *q;                    // [n] never null (the caller's array or scratch)
    float *tail;                 // [n] or null: no tail pass
    unsigned long long *cnt;     // [0] skipped, [1] incomplete, [2] (list != null only) scored with gaps, which [1] counted too: added to
    const uint32_t *list;        // null, or MissArgs::list of this range as launch_miss_list left it (DPMM_OPT_TYPICALITY_GAPS): behind the passes
    const unsigned long long *list_cnt;      // above, typ_gap_kernel rewrites q and tail of the listed points; [0] = entries of list
};
hipError_t launch_typicality_range(const TypicalityArgs &a, int max_grid, hipStream_t s);
// ---- per-feature explanation of a point (explain.hip; include/dpmm_hip_explain.h): behind launch_typicality_range of the same range, whose
// class words it reads: for a scored point g = R_k' R_k (x - m_k), the conditional residual, z-score and two-sided tail of every feature
constexpr int EXPLAIN_MAX_TOP = 16;       // DPMM_EXPLAIN_MAX_TOP
struct ExplainArgs {
    int64_t n;
    int K, D;
    const float *X;              // [n][ldx], the range's first point
    int64_t ldx;
    const float *Rt;             // as MissArgs::Rt
    const float *Rr;             // [K][D][miss_pitch(D)]: Rr[k][r][d] = R_k[r][d], zero below the diagonal (d < r) and in the pad (d >= D)
    const float *a;              // [K][miss_pitch(D)]: a[k][d] = sum_{r <= d} R_k[r][d]^2, summed in Float64 and rounded once; zero in the pad
    const float *mu;             // cluster k's mean: mu + k * mu_step
    int64_t mu_step;
    const double *cst;           // as MissArgs::cst: [k * MISS_CST] = df_k
    int32_t *cls;                // [n] the class words launch_typicality_range wrote for this range (read; with a list, explain_gap_kernel
                                 // adds r << 24 to a listed point's word for its tail pass)
    float *residual;             // [n][ld] or null
    float *zscore;               // [n][ld] or null
    float *feature_tail;         // [n][ld] or null
    int32_t *features;           // [n][ld] or null; written only if top > 0
    int top;                     // 0: all D features in order; else the top features of largest |zscore|, 1 <= top <= min(D, EXPLAIN_MAX_TOP)
    int64_t ld;                  // >= (top ? top : D)
    const uint32_t *list;        // null, or as TypicalityArgs::list: explain_gap_kernel rewrites the rows of the listed points
    const unsigned long long *list_cnt;
};
hipError_t launch_explain_params(const float *Rpk, int64_t step, float *Rr, float *a, int K, int D, hipStream_t s);      // Rpk: as launch_miss_transpose
hipError_t launch_explain_range(const ExplainArgs &a, int max_grid, hipStream_t s);
hipError_t launch_explain_gap_range(const ExplainArgs &a, int max_grid, hipStream_t s);      // explain_gap.hip: behind launch_explain_range, a.list != null
// ---- explanation by groups of features (explain_group.hip; include/dpmm_hip_explain_groups.h): behind launch_typicality_range of the same
// range: for a scored point and every group q_G = |W g_G|^2 and the tail of its F statistic
constexpr int EXPLAIN_MAX_GROUPS = 64;    // DPMM_EXPLAIN_MAX_GROUPS
constexpr int explain_group_pitch(int s) { return 64 * ((s + 63) / 64); }      // rows a column of a group's W is padded to
struct ExplainGroupArgs {
    int64_t n;
    int K, D, G;
    const float *X;              // [n][ldx], the range's first point
    int64_t ldx;
    const float *Rt;             // as ExplainArgs
    const float *Rr;
    const float *mu;
    int64_t mu_step;
    const double *cst;
    const int32_t *cls;          // [n] the class words launch_typicality_range wrote for this range
    const int32_t *goff;         // [G + 1] group j holds the entries goff[j] .. goff[j + 1] - 1 of gfeat
    const int32_t *gfeat;        // [goff[G]] 0-based features, below D
    const int64_t *gw;           // [G] the first word of group j inside a cluster's image of W
    const float *W;              // [K][wstep]: group j's column c at W + k * wstep + gw[j] + c * explain_group_pitch(s_j), entry r the
                                 // Float32 W_rc, zero above the diagonal (r < c) and in the pad (r >= s_j)
    int64_t wstep;
    float *group_q;              // [n][ld] or null
    float *group_tail;           // [n][ld] or null
    int64_t ld;                  // >= G
};
hipError_t launch_explain_group_range(const ExplainGroupArgs &a, int max_grid, hipStream_t s);
// draws of the missing features (include/dpmm_hip_impute.h) behind launch_miss_list and launch_miss_patch(a, false, ..) of the same range
constexpr int64_t MISS_DRAW_MAX = (int64_t)1 << 26;      // draw indices: 64 Philox blocks each in a 32-bit block number
struct MissDraw {
    float *out;                  // element (jd, i, f) of the range at out[jd * draw_stride + i * ld + f]: f < min(ld, draw_stride) is written
    int64_t ld, draw_stride;
    int32_t *comp;               // null, or comp[jd * comp_stride + i]: the 0-based drawn cluster of a listed point, -1 elsewhere
    int64_t comp_stride;
    uint64_t seed;
    int64_t i0;                  // global index of the range's first point
    int64_t draw0;               // draw index of jd = 0
    int ndraws;
};
hipError_t launch_miss_draw(const MissArgs &a, const MissDraw &w, int max_grid, hipStream_t s);
// ---- label trace (trace.hip; include/dpmm_hip_trace.h).  A row holds nvec 16-byte vectors of 8 ids, padded with 0xFFFF.
constexpr int TRACE_LDS_CELLS = 16384;    // 32-bit counters of a group of tables in LDS (64 KiB)
struct TracePair {                        // one table of a group
    const uint16_t *zt;                   // the column slot's row
    int Kt;
    unsigned cell0;                       // first cell of the table inside the group's LDS image
    unsigned long long *out;              // the table [Ks][Kt] in the device image of the result
};
struct TraceGroup {                       // consecutive pairs of one row slot, cells <= TRACE_LDS_CELLS
    const uint16_t *zs;
    int Ks, pair0, npairs, cells;         // pairs [pair0, pair0 + npairs) of the TracePair array
};
struct TraceConfSlot { const uint16_t *z; int K; unsigned off; };      // a listed slot of dpmm_trace_confidence: row, K, first float of its ratio table
hipError_t launch_trace_record(const int32_t *bins, int64_t n, uint16_t *row, int64_t nvec, hipStream_t s);
hipError_t launch_trace_tables(const TraceGroup *groups, int ngroups, const TracePair *pairs, int max_cells, int64_t nvec, hipStream_t s);
hipError_t launch_trace_pair_global(const uint16_t *zs, const uint16_t *zt, int Ks, int Kt, int64_t nvec, unsigned long long *out, hipStream_t s);
hipError_t launch_trace_confidence(const uint16_t *za, int Ka, const TraceConfSlot *slots, int ns, const float *ratio, int64_t n, int64_t nvec,
                                   float *out, hipStream_t s);
hipError_t launch_trace_read(const uint16_t *row, int64_t n, int64_t *labels, hipStream_t s);
// ---- drawing points (sample.hip; include/dpmm_hip_sample.h): n samples from global index i0; every output pointer is that of the call's
// first sample
struct SampleArgs {
    int64_t i0, n;
    const int64_t *cstart;    // [K + 1] device: first sample of every cluster relative to the call, clipped to [0, n]
    const int32_t *tstart;    // [K + 1] device, NIW: first 64-point tile of every cluster
    int K, D;
    uint64_t seed;
    const float *m;           // NIW [K][D]
    const float *At;          // NIW [K][D][D] TRANSPOSED: At[b][a] = A[a][b], zero where b < a
    const float *df;          // NIW [K]
    const uint32_t *thr;      // Multinomial [K][D]
    const int32_t *alias;     // Multinomial [K][D]
    int64_t trials;
    float *x;                 // dense [n][ld]
    int64_t ld;
    int64_t *labels;          // [n] or null
    int32_t *cnt;             // sparse, first pass: [n] stored entries of every sample
    const int64_t *colptr;    // sparse, second pass: [n + 1] absolute offsets
    int64_t *rowval;
    float *nzval;
    int64_t extent;           // entries behind rowval / nzval
};
hipError_t launch_sample_niw(const SampleArgs &a, int ntiles, int cus, hipStream_t s);
hipError_t launch_sample_mult_dense(const SampleArgs &a, hipStream_t s);
hipError_t launch_sample_mult_sparse(const SampleArgs &a, bool fill, hipStream_t s);
hipError_t launch_sample_add_i64(int64_t *p, int64_t n, int64_t v, hipStream_t s);
hipError_t launch_ingest_rows(float *dst, int64_t ldx, const void *src, int is_f64, int64_t ld, int64_t rows, int D, int nan_to_zero,
                              hipStream_t s);
hipError_t launch_copy_bytes(void *dst, const void *src, size_t bytes, hipStream_t s);
hipError_t launch_copy_bytes16(void *dst, const void *src, size_t bytes, hipStream_t s);   // 16-byte aligned dst / src, size rounded up to 16
hipError_t launch_init_labels(int32_t *bins, int64_t n, int64_t first_index, int init_clusters, int label0, uint64_t seed,
                              uint32_t epoch, hipStream_t s);
// step statistics: flags[k] = 1 when cluster k has an empty sub-cluster (counts: [2K] Int64, global), flags[K] = any;
// then re-draw the sub-labels of flagged clusters (reset_bad_clusters_worker!)
hipError_t launch_bad_flags(const int32_t *bin_total, const long long *global_counts, int K, uint8_t *flags, hipStream_t s);
hipError_t launch_widen_counts(const int32_t *src, int stride, long long *dst, int n, hipStream_t s);
hipError_t launch_gather_rows(float *dst, int64_t ld_dst, const float *src, int64_t ld_src, const int32_t *slot, int rows, int D, hipStream_t s);
hipError_t launch_bins_from_i64(int32_t *bins, const int64_t *labels, const int64_t *sub, int64_t n, hipStream_t s);
hipError_t launch_bins_to_i64(const int32_t *bins, int64_t *labels, int64_t *sub, int64_t n, hipStream_t s);
hipError_t launch_contingency(const int32_t *bins, const int32_t *gt, int64_t n, int K, int n_gt, unsigned long long *counts, hipStream_t s);
hipError_t launch_i64_to_i32(int32_t *dst, const int64_t *src, int64_t n, hipStream_t s);
// pairs: [2*m] = idx[0..m-1], new_idx[0..m-1] as 0-based Int32 cluster ids (device memory)
hipError_t launch_split(int32_t *bins, int64_t n, int64_t first_index, const int32_t *pairs, int m, uint64_t seed,
                        uint32_t epoch, hipStream_t s);
hipError_t launch_merge(int32_t *bins, int64_t n, const int32_t *pairs, int m, hipStream_t s);
hipError_t launch_remap(int32_t *bins, int64_t n, const int32_t *map, hipStream_t s);  // label k -> map[k]
hipError_t launch_reset_sub(int32_t *bins, int64_t n, int64_t first_index, const int32_t *idx, int m, uint64_t seed,
                            uint32_t epoch, hipStream_t s);

// ---- points in and out of caller-owned device memory (tensor_io.hip; include/dpmm_hip_tensor.h)
// dtype: the DPMM_DT_* code; source element (point i, feature d) at src + (i * stride_point + d * stride_feature) elements, strides >= 0.
// Writes dst [n][ldx] whole, pad columns [D, ldx) included (ldx a multiple of 4, dst 16-byte aligned).
enum { INGEST_POINT_MAJOR = 0, INGEST_FEATURE_MAJOR = 1, INGEST_GENERAL = 2 };
size_t ingest_elem_size(int dtype);      // 0: unknown code
int ingest_mode(const void *src, int dtype, int64_t stride_point, int64_t stride_feature, int64_t n, int D);      // the access pattern the launcher takes
hipError_t launch_ingest_strided(float *dst, int64_t ldx, const void *src, int dtype, int64_t stride_point, int64_t stride_feature, int64_t n, int D,
                                 int nan_to_zero, hipStream_t s);
// out [n][ld_out] (ld_out >= D, columns [D, ld_out) = 0) from the Float32 image X, else from the byte copy X8, else zeros
hipError_t launch_points_readback(float *out, int64_t ld_out, const float *X, int64_t ldx, const uint8_t *X8, int64_t ld8, int64_t n, int D,
                                  hipStream_t s);
hipError_t launch_sparse_readback(float *out, int64_t ld_out, const int64_t *cp, const uint16_t *ri, const float *val, int64_t n, hipStream_t s);

// ---- wide points projected to the ctx's dimension while they are read (project.hip; include/dpmm_hip_project.h)
// Wimg: [ceil(D_in / 32)][proj_njb(D)][3 planes][64 lanes] 16-byte words -- lane l: the bf16 W[32 s + 8 (l >> 4) + e][16 jb + (l & 15)], e < 8, zero
// outside [D_in][D]; bias: [16 proj_njb(D)] Float32, b[j] (+0 for j >= D).  Writes dst [n][ldx] whole; the source as launch_ingest_strided's.
constexpr int PROJ_BLOCK = 256;
int proj_njb(int D);               // blocks of 16 output columns a workgroup carries: 4, 8 or 16
int proj_tile_points(int D);       // points per workgroup: 512, 256 or 128
hipError_t launch_project(float *dst, int64_t ldx, int D, const void *src, int dtype, int64_t stride_point, int64_t stride_feature, int64_t n, int D_in,
                          const void *Wimg, const float *bias, hipStream_t s);

// ---- sparse points out of caller-owned device memory (csc_io.hip; include/dpmm_hip_csc.h)
// cp: n + 1 ABSOLUTE offsets (minus base) into rv / nz, Int32 or Int64 as rv; nz of the DPMM_DT_* type value_dtype; extent: entries behind rv / nz.
// bad[0] (preset to ~0): min over the offenders of point << 20 | (position in the column + 1) << 3 | reason
enum { CSC_BAD_RANGE = 1, CSC_BAD_ORDER = 2, CSC_BAD_DECREASES = 3, CSC_BAD_OUTSIDE = 4 };
constexpr int CSC_SCAN_TILE = 2048;      // points per workgroup and pass of the offsets' scan
inline int64_t csc_scan_tiles(int64_t n) { return (n + CSC_SCAN_TILE - 1) / CSC_SCAN_TILE; }
hipError_t launch_csc_dev_check(const void *cp, const void *rv, const void *nz, int index_i64, int value_dtype, int64_t n, int64_t extent, int D, int base,
                                int32_t *cnt, unsigned long long *bad, hipStream_t s);
hipError_t launch_csc_scan(const int32_t *cnt, int64_t n, int64_t *bt /* [csc_scan_tiles(n) + 1] */, int64_t *cp_out /* [n + 1] */, hipStream_t s);
hipError_t launch_csc_dev_compact(const void *cp, const void *rv, const void *nz, int index_i64, int value_dtype, int64_t n, int base, const int64_t *cp_out,
                                  uint16_t *ri, float *val, hipStream_t s);

// ---- stable counting sort of the points by bin + segmented statistics (suffstats.hip)
constexpr int SORT_TILE = 2048;  // points per sorting wave of big shards (SortBufs::tile: 2048 or SORT_TILE_SMALL)
constexpr int SORT_TILE_SMALL = 512;
constexpr int FAST_TOTAL_STRIDE = 32;   // ints between the running totals of two bins (one 128-byte line per bin: the histogram adds with atomics)

struct SortBufs {
    int tile;             // points per sorting wave of this context's passes: SORT_TILE or SORT_TILE_SMALL
    int32_t *tile_hist;   // [nbins][ntiles_sort] exclusive prefix over the tiles of a bin (written by the scan from tile_cnt)
    int32_t *tile_cnt;    // [nbins][ntiles_sort] points of bin b in tile t (written by the histogram)
    int32_t *spec_bins;   // [n] the re-drawn bin of every point whose cluster was one-sided in the point's tile (written by hist_kernel<.., SPEC>, read by the scatter for flagged clusters)
    int32_t *tile_spec;   // [min(nbins, STEP_SPEC_MAX_BINS)][ntiles_sort] the same counts with the bad-cluster reset of the tile's one-sided clusters counted ahead (hist_kernel<.., SPEC>)
    int32_t *fast_total;  // [nbins][FAST_TOTAL_STRIDE] (element 0 of each line) running bin totals of the per-step histogram (integer atomics), cleared by scan_starts_kernel
    unsigned *ticket;     // [1] unused since the per-step scan and the starts are two launches (kept: the buffers are allocated as a set)
    uint16_t *prev_lab;   // [n] cluster label of every point at the previous per-step pass (0xFFFF: none yet); null: no tracking
    uint8_t *cdirty;      // [DPMM_MAX_CLUSTERS_K + 1] a point entered or left cluster k since then; last element: every cluster
    uint8_t *cmode;       // [DPMM_MAX_CLUSTERS_K] per-step pass: 0 both sub-clusters computed, 1 / 2 left / right derived from the cached cluster row
    int32_t *bin_total;   // [nbins]
    int32_t *bin_start;   // [nbins + 1]
    int32_t *perm;        // [n]
    int32_t *item_start;  // [nbins + 1]
    uint8_t *bin_sel;     // [nbins] 1 = compute statistics for this bin
    int32_t *perm_total;  // [1] number of points placed in perm by the last sort (== n when every label was in range)
};

hipError_t launch_sort_by_bin(const int32_t *bins, int64_t n, int nbins, const SortBufs &b, hipStream_t s);
constexpr int STEP_SPEC_MAX_BINS = 512;      // bins (2K) up to which the per-step histogram counts the bad-cluster reset ahead (a second set of LDS counters per tile)
struct StepReset { const long long *global_counts; uint8_t *flags; int K; uint8_t *cside; int64_t first; uint64_t seed; uint32_t epoch; };
hipError_t launch_step_hist(const int32_t *bins, int64_t n, int nbins, const SortBufs &b, hipStream_t s, int spec = 0, int64_t first = 0, uint64_t seed = 0, uint32_t epoch = 0);
hipError_t launch_step_reset(int32_t *bins, int64_t n, int64_t first, int nbins, const SortBufs &b, const long long *global_counts, uint8_t *flags,
                             int K, uint64_t seed, uint32_t epoch, uint8_t *cside, hipStream_t s);     // cside != null: speculative reset of this shard's candidates
// rows [2K][stride] of the speculatively reset labels -> red [3K][stride] (the travelling rows of the one-collective pass; Multinomial: its reduce does not write them itself)
hipError_t launch_onecoll_rows(const double *rows, double *red, int64_t stride, int K, const uint8_t *cside, uint8_t *flags, hipStream_t s);
hipError_t launch_niw_finalize_rows(const double *red, double *out, int64_t stride, int K, const uint8_t *cside, uint8_t *flags, uint8_t *flags_host, hipStream_t s);
hipError_t launch_niw_undo_reset(int32_t *bins, int64_t n, int K, const uint8_t *flags, const uint8_t *cside, hipStream_t s);
struct StatsArgs;
hipError_t launch_sort_finish(const int32_t *bins, const StatsArgs &a, hipStream_t s);
hipError_t launch_step_scan_scatter(int32_t *bins, const StatsArgs &a, int derive, int force_all, int fused_starts, const StepReset *rs, hipStream_t s);
hipError_t launch_derive_rows(double *out, double *cache, const uint8_t *mode, uint8_t *dirty, int64_t stride, int K, const uint8_t *flags_src,
                              uint8_t *flags_dst, hipStream_t s);

struct StatsArgs {
    const float *X;
    int64_t ldx;
    int64_t n;
    int D;
    int nbins;
    int chunk;             // points per work item
    int max_items;
    int range_groups;      // NIW: workgroups of the statistics kernel; each owns a contiguous range of items (0: one item per workgroup)
    SortBufs sb;
    double *slabs;         // NIW: [NIW_STATS_MAX_GROUPS + nbins][slab_stride] (slots, suffstats.hip head_slot); Multinomial: [max_items][slab_stride]
    int64_t slab_stride;
    double *out;           // packed [nbins][packed_stride]
    int64_t packed_stride;
    const int32_t *row_off; // NIW: [packed_stride] packed-row element -> position inside a slab (launch_niw_row_offsets)
    const int32_t *inv_off; // NIW: [slab_stride] slab position -> packed-row element (-1: none), the inverse table
    // NIW per-step pass with derived statistics: the reduce kernel forms the rows that were not computed (null mode: plain reduce)
    const uint8_t *mode;    // [K] 0 both computed -> cache = left + right, 1 / 2: left / right = cache - computed
    double *cache;          // [K][packed_stride]
    uint8_t *dirty;         // [DPMM_MAX_CLUSTERS_K + 1] cleared for the next pass
    const uint8_t *flags_src; uint8_t *flags_dst; int K;    // rider: bad-cluster flags -> the caller's pinned block (null: none)
    // one-collective per-step pass: `out` has 3K rows -- [2K rows of the labels as swept | K re-drawn left rows] -- cside [K] says which
    // clusters' sub-labels were reset speculatively on this shard (suffstats.hip reset_recount_kernel); zero2 = two flag bytes to clear
    const uint8_t *cside; uint8_t *zero2;
};
// (NIW_STATS_MAX_GROUPS, the workgroups of the NIW statistics kernel at most -- slab slots = this + 2 K -- comes from stats_ranges.h)
int64_t niw_slab_stride(int D);
hipError_t launch_niw_row_offsets(int32_t *row_off, int32_t *inv_off, int D, int64_t packed_stride, hipStream_t s);
int64_t mult_slab_stride(int D);
hipError_t launch_niw_stats(const StatsArgs &a, hipStream_t s);
hipError_t launch_mult_stats(const StatsArgs &a, hipStream_t s);
hipError_t launch_mult_stats_u8(const StatsArgs &a, const uint8_t *X8, int64_t ld8, hipStream_t s);

// ---- the Multinomial master's draws on the device (mult_master.hip) ----
#define DPMM_MULT_MASTER_MAXD 16384      // the row's log Gamma variates live in LDS (8 bytes each)
hipError_t launch_mult_dirichlet(const double *rows, int64_t stride, const float *alpha0, const float *alpha1, int outlier_first, int D, int64_t ldx,
                                 int K, uint64_t seed, uint32_t epoch, float *raw, hipStream_t s);
#define DPMM_MULT_MASTER_MAXPAIRS 8192
hipError_t launch_mult_marginals(const double *rows, int64_t stride, const float *alpha0, const float *alpha1, int outlier_first, int D, int K,
                                 const int32_t *pairs, int npairs, const double prior_c[4], double *out, hipStream_t s);

// ---- the master's dense maths on the device (niw_master.hip) ----
#define DPMM_MASTER_MAXD 256
#ifndef DPMM_MASTER_NSCALARS
#define DPMM_MASTER_NSCALARS 8      // doubles per distribution in the scalar records: N, kappa', nu', log det(nu' psi'), log Gamma_D(nu' / 2), 3 spare (dpmm_hip.h)
#endif
struct NiwMasterArgs {
    int D, DP;                    // DP = 16 * ceil(D / 16)
    int64_t packed_stride;
    double kappa0, nu0;
    const double *m0;             // [D]
    const double *psi_lo;         // prior psi, symmetrised, packed lower triangle [D (D + 1) / 2]
    double *fac;                  // [rows][DP][DP]  P = nu' psi' -> its factor L (row = 3 slot + w)
    double *mean;                 // [rows][DP]      m'
    double *kap, *nu;             // [rows]
    double *rows_store;           // [slots][2][packed_stride]  statistics of every slot (left, right)
    float *mu_draw;               // [3 K][DP]       the current draws' means (cluster order)
    uint64_t seed;
};
size_t niw_master_lds_bytes(int DP);
hipError_t launch_niw_master_pairs(const NiwMasterArgs &a, const int32_t *pairs, int n, double *scratch, double *small, hipStream_t s);
hipError_t launch_niw_rows_gather(const double *rows_store, const int32_t *slots, int n, int64_t stride, double *dst, hipStream_t s);
hipError_t launch_niw_master_posterior(const NiwMasterArgs &a, const int32_t *jobs, int njobs, const double *rows, double *small, hipStream_t s);
bool niw_master_can_fuse_pairs(const NiwMasterArgs &a);
hipError_t launch_niw_master_posterior_pairs(const NiwMasterArgs &a, const int32_t *jobs, int njobs, const double *rows, double *small,
                                             const int32_t *cluster_pairs, int npairs, double *pair_small, hipStream_t s,
                                             int noise_nmat = 0, uint32_t noise_epoch = 0, double *noise_Y = nullptr);   // noise_Y: also the standard normals of the draws that follow (round 6)
hipError_t launch_niw_draw_inputs(const NiwMasterArgs &a, const int32_t *slot_of_cluster, int K, uint32_t epoch, double *Aout, double *xiout, hipStream_t s);
hipError_t launch_niw_master_noise(const NiwMasterArgs &a, int nmat, uint32_t epoch, double *Y, hipStream_t s);
hipError_t launch_niw_master_draw(const NiwMasterArgs &a, const int32_t *slot_of_cluster, int K, uint32_t epoch, double *Y, float *logdet_sigma,
                                  const float *lr, const float *wts, float *Rp, float *mup, float *cst, float *tail, int NB,
                                  unsigned long long *work, int what, hipStream_t s);

// Test hook (dpmm_debug_set_prelaunch_hook): called on the host in front of EVERY kernel launch of the library.  tests/tools/poison.py
// installs a function that waits for the device and refills the LDS and the register files of every CU with a NaN pattern, so that a
// kernel reading LDS or registers it never wrote sees that instead of the (finite) leftovers of the library's own previous kernel.
extern void (*g_prelaunch)(void *);
extern void *g_prelaunch_arg;
inline void prelaunch() { if (g_prelaunch) g_prelaunch(g_prelaunch_arg); }
#define DPMM_LAUNCH(...) do { ::dpmm::prelaunch(); hipLaunchKernelGGL(__VA_ARGS__); } while (0)

}  // namespace dpmm
