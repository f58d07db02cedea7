// dpmm_api.cpp -- C ABI of libdpmmhip.so (see include/dpmm_hip.h -- and its companions dpmm_hip_master.h, dpmm_hip_debug.h -- for the contract and the
// reference functions each entry point replaces).  Host-side glue only: device memory
// ownership, parameter staging, kernel sequencing on ONE stream, error mapping.
// There is no CPU fallback anywhere in this file: without a usable gfx950 device
// dpmm_create fails with DPMM_ENODEVICE.
#include "../../include/dpmm_hip.h"
#include "../../include/dpmm_hip_master.h"
#include "../../include/dpmm_hip_debug.h"
#include "../../include/dpmm_hip_tensor.h"
#include "../../include/dpmm_hip_csc.h"
#include "../../include/dpmm_hip_score.h"
#include "../../include/dpmm_hip_rank.h"
#include "../../include/dpmm_hip_overlap.h"
#include "../../include/dpmm_hip_batchstats.h"
#include "../../include/dpmm_hip_countstats.h"
#include "../../include/dpmm_hip_typicality.h"
#include "../../include/dpmm_hip_explain.h"
#include "../../include/dpmm_hip_explain_groups.h"
#include "../../include/dpmm_hip_holdout.h"
#include "../../include/dpmm_hip_countholdout.h"
#include "../../include/dpmm_hip_trace.h"
#include "../../include/dpmm_hip_missing.h"
#include "../../include/dpmm_hip_impute.h"
#include "../../include/dpmm_hip_regress.h"
#include "../../include/dpmm_hip_regress_draw.h"
#include "../../include/dpmm_hip_regress_cdf.h"
#include "../../include/dpmm_hip_recommend.h"
#include "../../include/dpmm_hip_count_explain.h"
#include "../../include/dpmm_hip_sample.h"
#include "../../include/dpmm_hip_project.h"

#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <ctime>
#include <string>
#include <unordered_map>
#include <vector>

#include "dpmm_kernels.h"
#include "project_image.h"
#include "typicality_math.h"      // typ_log_beta, for the density constants of dpmm_set_regression_levels
#include "dev_mem.h"      // DevBuf / PinBuf: every buffer below is a member or a local of these and is never freed by hand

namespace dpmm {      // test hook in front of every kernel launch (dpmm_kernels.h DPMM_LAUNCH, dpmm_debug_set_prelaunch_hook)
void (*g_prelaunch)(void *) = nullptr;
void *g_prelaunch_arg = nullptr;
}
using namespace dpmm;

static_assert(DPMM_MAX_CLUSTERS == DPMM_MAX_CLUSTERS_K, "header / kernel limits out of sync");

#ifdef DPMM_STAMPS
static unsigned long long *g_dbg = nullptr;
#endif
namespace {
thread_local std::string g_create_error;

int nb_for_dim(int D) { return D <= 16 ? 1 : D <= 32 ? 2 : D <= 64 ? 4 : D <= 128 ? 8 : 16; }
}  // namespace

// What the *_begin of an accumulation over the score table (overlap, batchstats, holdout, countstats, countholdout) leaves for its _accumulate and _read calls
struct AccSession {
    bool active = false;
    int K = 0, mode = 0, floor = 0;      // K at the begin; the begin's arguments (overlap has none)
    float min_logdens = 0.f;
    unsigned long long gen = 0;          // pred_gen at the begin
    int use2 = 0;                        // the second floor: the tail (NIW) or the log-density per count (Multinomial); the holdouts take it
    float min2 = 0.f;                    // at their begin, the statistics by their set call, between the begin and the first _accumulate
    bool accumulated = false;            // an _accumulate has run since the begin
};

struct dpmm_ctx {
    int prior = 0, D = 0, device = 0;
    int64_t n = 0, first = 0, ldx = 0;
    uint64_t seed = 0;
    int NB = 0;          // NIW: 16-blocks per dimension
    int tile = 0;        // points per sweep workgroup tile
    int64_t ntiles = 0;
    int cus = 256;
    int sweep_grid = 0, sweep_grid_max = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_part[2] = {nullptr, nullptr};   // DPMM_OPT_KERNEL_TIMING bit 3: behind niw_lean_kernel / behind the LSTORE sweep kernel (dpmm_last_sweep_parts_ms)
    int have_parts = 0;                           // 0: no three-kernel sweep timed yet; 1: labels + sub-labels (no lean kernel); 2: lean + labels + sub-labels
    bool have_sweep_ev = false, have_stats_ev = false;

    DevBuf<float> dX;
    DevBuf<int32_t> dbins;
    bool have_points = false, have_labels = false;
    DevBuf<int32_t> d_gt;  // ground truth of the shard (on-device evaluation)
    int n_gt = 0;
    DevBuf<unsigned long long> d_cont;
    bool have_perm = false;   // sb.perm holds a permutation of [0,n) sorted by a recent labelling

    // parameters
    int K = 0, Kcap = 0;
    DevBuf<float> d_raw;   // NIW: R [3K][D][D] ; MULT: unused
    DevBuf<float> d_mu;    // NIW raw mu [3K][D]
    DevBuf<float> d_Rp;    // NIW packed fragments / MULT packed logp
    DevBuf<float> d_mup;   // NIW padded mu
    DevBuf<float> d_cst;   // [3K]
    DevBuf<uint32_t> d_Lp16;  // MULT: 3-plane bf16 split of the log-probabilities (count data fast path)
    // MULT, device master: the NEXT parameter draws, made right behind the per-step statistics (while the host decides splits and merges) into
    // a second set of buffers; dpmm_mult_master_draw swaps the sets when its epoch / K / outlier flag are the ones guessed and the rows have
    // not changed since (else it draws as before)
    DevBuf<float> d_raw2, d_Rp2;
    DevBuf<uint32_t> d_Lp16_2;
    bool mspec_valid = false;
    bool rp_current = true, rp2_current = true;   // the Float32 fragment image (d_Rp / d_Rp2) matches d_raw / d_raw2: the device master skips it for byte / bf16 data; the Float32 sweep packs it on demand
    uint32_t mspec_epoch = 0, mdraw_epoch = 0;
    int mspec_K = 0, mspec_outlier = 0, opt_mult_draws_ahead = 1;
    bool mdraw_seen = false;           // a dpmm_mult_master_draw has run: its epoch + 1 is the guess
    long long mspec_used = 0;          // draws taken from the set made ahead (dpmm_debug / tests)
    hipEvent_t ev_rows = nullptr;      // dpmm_step_stats: rows and flags are in the pinned block (the draws launched ahead follow it)
    bool rows_on_demand = false, rows_late = false;   // dpmm_mult_master_rows_on_demand: with draws launched ahead the rows reach the pinned block BEHIND them
    // dpmm_mult_master_draw re-uses its pinned weights once the host has waited for the main stream (or for ev_rows, recorded later on it) since
    // the copy that read them -- a generation count instead of an event of its own (an event record costs ~5 us of stream time in front of the sweep)
    unsigned long long sync_gen = 0, cst_gen = 0;
    bool cst_inflight = false;
    bool marg_behind_ev = false;       // the log-marginals in the pinned block were complete at ev_rows (no need to wait for the stream)
    int x_bf16_exact = 0;     // MULT: every x is exactly representable in bf16 (checked at upload)
    DevBuf<uint8_t> dX8;   // MULT: byte copy of the points when every x is an integer in [0, 255] ([n][ld8])
    int64_t ld8 = 0;
    int x_u8 = 0;
    int opt_no_u8 = 0;
    // MULT: the points as compressed sparse columns (dpmm_upload_points_csc; mult_sparse.hip) -- then dX / dX8 are not allocated, and d_Rp / d_Rp2
    // hold the TRANSPOSED parameter image [D][3K] the sparse sweep reads (rp_current stays false: the Float32 fragment image is not kept)
    int x_sparse = 0;
    DevBuf<int64_t> d_cp;
    DevBuf<uint16_t> d_ri;
    DevBuf<float> d_val;
    int64_t nnz = 0;
    int chunk_dense = 512;            // points per statistics item while the points are dense (`chunk` is the one in use: set_points_chunk)
    bool repack_pending = false;      // a dense upload replaced sparse points: the dense kernels' parameter images are made from the raw rows
    DevBuf<float> d_scratch;
    int64_t scratch_stride = 0;
    bool have_params = false;
    DevBuf<float> d_lam, d_mdist, d_tail;   // NIW screening constants (per sweep)
    bool have_screen_prep = false, have_tail = false;
    DevBuf<float> d_tdf;   // Student-t constants of the predictive mode ([3K][2]) or null
    bool predictive = false;
    // scoring (include/dpmm_hip_score.h): one slab of the table and, for the host variant, the slab's outputs; allocated on first use, grown on demand
    DevBuf<float> d_score_table;
    DevBuf<char> d_score_out;
    double opt_score_mb = 128.0;       // DPMM_OPT_SCORE_TABLE_MB
    // exemplars (include/dpmm_hip_rank.h): running lists | counters | candidate counters; the candidate buffers; the staging of dpmm_rank_read
    DevBuf<unsigned long long> d_rank_state;
    DevBuf<char> d_rank_cand, d_rank_out;
    bool rank_active = false;
    int rank_m = 0, rank_which = 0, rank_K = 0, rank_parity = 0;
    int64_t rank_cap = 0;
    // cluster overlap (include/dpmm_hip_overlap.h): overlap | mass | counters; (M, S) of the points of one range; the chunk partials
    DevBuf<double> d_ov_acc;
    DevBuf<float2> d_ov_ms;
    DevBuf<double> d_ov_part;
    AccSession ov;
    // batch statistics (include/dpmm_hip_batchstats.h): N | sums | S | counters; two floats per point of one range; the chunk partials
    DevBuf<double> d_bs_acc;
    DevBuf<float2> d_bs_ms;
    DevBuf<double> d_bs_part;
    AccSession bs;
    // calibrated outlier scores (include/dpmm_hip_typicality.h): class word and q per point of one range, the two counters; the tails of one
    // range for the hold-out of dpmm_batchstats_set_min_tail (allocated only when it is in use)
    DevBuf<int32_t> d_typ_cls;
    DevBuf<float> d_typ_q;
    DevBuf<unsigned long long> d_typ_cnt;
    DevBuf<float> d_bs_tail;
    // per-feature explanations (include/dpmm_hip_explain.h): the row-major factors and the diagonals of R'R, allocated by the first explain
    // call and made from the parameter set exp_gen (0: none)
    DevBuf<float> d_exp_rr, d_exp_a;
    unsigned long long exp_gen = 0;
    // explanation by groups (include/dpmm_hip_explain_groups.h): the Float32 image of W, the descriptors (goff [G + 1], then gfeat) and the
    // groups' first words, allocated by dpmm_set_explain_groups and made for the parameter set exg_gen (0: none)
    unsigned long long exg_gen = 0;
    int exg_G = 0;
    int64_t exg_wstep = 0;
    DevBuf<float> d_exg_w;
    DevBuf<int32_t> d_exg_desc;
    DevBuf<int64_t> d_exg_gw;
    // held-out points (include/dpmm_hip_holdout.h): ballots, class counts and first slots of the workgroups of one range; the running totals;
    // the caller's destination as dpmm_holdout_begin took it.  With a tail floor the tails of a range go through d_bs_tail, as batchstats' do.
    DevBuf<unsigned long long> d_ho_ballot, d_ho_state;
    DevBuf<unsigned> d_ho_count;
    DevBuf<int64_t> d_ho_off;
    AccSession ho;
    float *ho_points = nullptr;
    int64_t *ho_index = nullptr;
    int64_t ho_cap = 0;
    // count statistics (include/dpmm_hip_countstats.h): N | sums | counters; two floats per point of one range; the chunk partials
    DevBuf<double> d_cs_acc;
    DevBuf<float2> d_cs_ms;
    DevBuf<double> d_cs_part;
    AccSession cs;
    // the floor per count (dpmm_countstats_set_per_count): the Float64 totals of the points of one range, allocated only when a floor per
    // count is in use and shared with the collection below
    DevBuf<double> d_cs_tot;
    // held-out count points (include/dpmm_hip_countholdout.h): ballots, class counts and first slots go through d_ho_ballot / d_ho_count /
    // d_ho_off (a ctx has one prior); the workgroups' entry counts and first entry offsets; the running totals; the caller's destination
    DevBuf<unsigned long long> d_ch_ent, d_ch_state;
    DevBuf<int64_t> d_ch_eoff;
    AccSession ch;
    dpmm_countholdout_dst ch_dst = {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
    // label trace (include/dpmm_hip_trace.h): slots rows of trace_nvec 16-byte vectors of ids; K per slot (0: never recorded); the device
    // images of a call's tables, descriptors, ratio tables and confidence
    DevBuf<uint16_t> d_trace;
    int trace_slots = 0;
    int64_t trace_nvec = 0;
    std::vector<int> trace_K;
    DevBuf<unsigned long long> d_trace_counts;
    DevBuf<char> d_trace_desc;
    DevBuf<float> d_trace_ratio, d_trace_conf;
    // missing features (include/dpmm_hip_missing.h): the constants of the marginals on the host (formed by dpmm_set_predictive_niw); on the
    // device, allocated by the first call that marginalises: their copy, the transposed factors, a range's list and the three counters
    int opt_score_missing = 0;         // DPMM_OPT_SCORE_MISSING
    int opt_typ_gaps = 0;              // DPMM_OPT_TYPICALITY_GAPS
    std::vector<double> h_miss_cst;    // [K][MISS_CST]
    int miss_slots = 0;                // slots of the parameter staging when the predictive parameters were committed (their layout in d_par)
    unsigned long long pred_gen = 0, miss_gen = 0;      // parameter set in force / the one the device copies were made from (0: none)
    DevBuf<float> d_miss_rt;
    DevBuf<double> d_miss_cst;
    DevBuf<uint32_t> d_miss_list;
    DevBuf<unsigned long long> d_miss_cnt;
    bool miss_counted = false;         // the last table call marginalised: the counters hold its counts
    // mixture regression (include/dpmm_hip_regress.h): the Float32 tables of dpmm_set_regression, made for the parameter set reg_gen (0: none);
    // the per-tile counts of the points that take no part, of one range, allocated by the first dpmm_regress_points
    int reg_Dt = 0;
    bool reg_no_var = false;           // a cluster has df + D <= 2: no variance
    unsigned long long reg_gen = 0;
    DevBuf<float> d_reg_bt, d_reg_c, d_reg_v;
    DevBuf<double> d_reg_hd;
    DevBuf<unsigned> d_reg_skip;
    // draws of the targets (include/dpmm_hip_regress_draw.h): cluster k's image B_k' on top of W_k', allocated by dpmm_set_regression_factor;
    // in force while reg_factor is set and the regression tables are (dpmm_set_regression clears it)
    bool reg_factor = false;
    DevBuf<float> d_reg_bw;
    DevBuf<int32_t> d_reg_kc;          // [batch][P] drawn clusters and scales of a batch of draws of one range (at most 16 MiB together),
    DevBuf<float> d_reg_sc;            // allocated by the first dpmm_regress_draw_points
    // conditional quantiles (include/dpmm_hip_regress_cdf.h): levels [L], z [K][L], log densities at 0 [K], made by dpmm_set_regression_levels
    // for the parameter set reg_lev_gen (0: none; dpmm_set_regression clears it)
    unsigned long long reg_lev_gen = 0;
    int reg_L = 0;
    DevBuf<double> d_reg_lev;
    // next-count probabilities (include/dpmm_hip_recommend.h): the padded Float32 image of theta, made by dpmm_set_recommend for the parameter
    // set rec_gen (0: none); the per-tile counts of the points that take no part, of one range, allocated by the first dpmm_recommend_points
    unsigned long long rec_gen = 0;
    DevBuf<float> d_rec_theta;
    DevBuf<unsigned> d_rec_skip;
    // surprising features (include/dpmm_hip_count_explain.h): log theta and log1p(-theta), [K][D] each, and the order, [K][D], made by
    // dpmm_set_count_explain for the parameter set cex_gen (0: none); the per-tile counts of the skipped and the incomplete points of one range
    unsigned long long cex_gen = 0;
    DevBuf<double> d_cex_log;
    DevBuf<int32_t> d_cex_order;
    DevBuf<unsigned> d_cex_skip, d_cex_inc;
    DevBuf<double> d_cex_tot;      // ... and their totals and 0-based labels, for the tail kernel
    DevBuf<int32_t> d_cex_lab;
    // drawing points (include/dpmm_hip_sample.h): the sampler's tables (dpmm_set_sampler_*) and what a call needs beside its outputs
    // (cluster and tile starts; sparse: 4 bytes per point of counts and the scan's tile totals), allocated on first use
    DevBuf<float> d_sm_m, d_sm_At, d_sm_df;
    DevBuf<uint32_t> d_sm_thr;
    DevBuf<int32_t> d_sm_alias;
    int sm_K = 0;
    DevBuf<int64_t> d_sm_cstart; DevBuf<int32_t> d_sm_tstart; int sm_start_cap = 0;
    DevBuf<int32_t> d_sm_cnt; DevBuf<int64_t> d_sm_bt;
    // projection (include/dpmm_hip_project.h): D_in (0: none), the plane image of W and -b as project.hip reads them, the host call's staging rows
    int proj_Din = 0;
    DevBuf<void> d_proj_W;
    DevBuf<float> d_proj_bias, d_proj_stage;

    // sort + stats
    SortBufs sb{};          // a view for the kernels; its arrays are owned by the members of sort_mem (filled by dpmm_create and DPMM_OPT_SORT_TILE)
    struct {
        DevBuf<int32_t> tile_hist, tile_cnt, spec_bins, tile_spec, fast_total, bin_total, bin_start, perm, item_start, perm_total;
        DevBuf<unsigned> ticket;
        DevBuf<uint16_t> prev_lab;
        DevBuf<uint8_t> cdirty, cmode, bin_sel;
    } sort_mem;
    int nt_sort = 0;          // tiles the sort tables are allocated for
    int sort_tile_min = SORT_TILE;   // smallest sort tile the tables can hold
    int chunk = 512;
    int max_items = 0;
    DevBuf<double> d_slabs;
    int64_t slab_stride = 0;
    DevBuf<int32_t> d_row_off;      // NIW: packed-row element -> slab position
    DevBuf<int32_t> d_inv_off;      // NIW: slab position -> packed-row element (reduce kernel)
    DevBuf<double> d_out;
    int64_t packed_stride = 0;
    DevBuf<double> d_proj, d_vals, d_smart;   // smart splits: projections [n], compacted copy [n], partials + v + mu
    DevBuf<int32_t> d_small;  // index lists for relabel kernels (Int32, <= 4*DPMM_MAX_CLUSTERS)
    std::vector<uint8_t> h_sel;
    // pinned host staging for every per-step transfer (pageable copies stall for tens of ms now and then)
    PinBuf<char> h_pin;
    // parameter staging (dpmm_params_staging): slot-indexed rows the host writes in place; the pack kernels read it directly
    PinBuf<char> h_par;
    int par_slots = 0;
    // statistics output (dpmm_step_stats / dpmm_suffstats_host): packed rows + flags, read by the host in place
    PinBuf<char> h_out;
    DevBuf<char> d_par;             // device copy of the staging's mu | R regions (NIW): the pack kernel gathers from HBM, not over the host link
    bool work_zeroed = false;          // the pack kernel cleared d_work and no sweep has run since
    int sel_all_ones = 0, sel_capacity = 0;   // sb.bin_sel[0..sel_all_ones) are known to be 1 (full passes skip the memset)
    DevBuf<long long> d_counts64;   // [2 * DPMM_MAX_CLUSTERS] global sub-cluster occupancies (multi-GPU)
    // Multinomial master on the device (mult_master.hip): priors, and how many clusters' complete rows the last statistics pass left in d_out
    DevBuf<float> d_malpha;         // [2][ldx]: cluster prior | outlier prior
    bool mult_master = false, mult_has_alpha1 = false;
    int rows_full_K = -1;
    // ... and its log-marginals (mult_marginal_kernel): prior constants {sum a, sum lgamma(a)} x 2, the pair list asked for ahead of the
    // next per-step pass, the pinned result block [3K][2] (N, L) | [pairs] and what it currently answers
    double mult_prior_c[4] = {0, 0, 0, 0};
    DevBuf<int32_t> d_mpairs;
    std::vector<int32_t> mpairs_req, mpairs_shadow;
    bool marg_req = false, marg_valid = false;
    int marg_req_outlier = 0, marg_K = 0, marg_np = 0;
    PinBuf<double> h_marg;
    // derived sub-cluster statistics of the per-step pass (derive_rows_kernel): cached cluster-level rows + label tracking
    DevBuf<double> d_ccache;        // [Kcap][packed_stride] left + right of every cluster as of the last pass that computed both
    bool cache_force = true;           // the next per-step pass computes every cluster in full (points uploaded, cache re-allocated, K changed)
    int cache_K = -1;
    int opt_derive = 1;
    int64_t dbg_early_wait = 0;        // event waits that returned before the posteriors' records were in host memory (dpmm_debug_counters)
    int opt_noise_ahead = -1;          // normals of the next draws on the second stream beside the sweep (DPMM_OPT_NOISE_AHEAD): -1 = for D >= 128 or shards below 4e6 points
    // device master (niw_master.hip)
    bool master = false;
    NiwMasterArgs ma{};                            // a view for the kernels: fac .. rows_store point into master_mem (master_capacity), m0 / psi_lo at d_m0 / d_psi_lo
    struct { DevBuf<double> fac, mean, kap, nu, rows_store; } master_mem;
    DevBuf<double> d_m0, d_psi_lo, d_pairs;
    DevBuf<double> d_Y[2];                         // draw outputs, two sets: [draw_cur] belongs to the parameters in use, the other takes the next draws
    DevBuf<float> d_mu_draw[2];
    int draw_cur = 0;
    size_t pair_cap = 0;                           // matrices in d_pairs (pooled pair scratch)
    DevBuf<float> d_ld_sigma[2];
    int master_slots = 0, master_K = 0;            // capacities: slots (fac / mean / rows_store), clusters (Y / mu_draw)
    // draws launched ahead (dpmm_step_master_device): a second stream, so that the pair kernels of the merge proposals do not queue behind them
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_master = nullptr, ev_spec = nullptr;      // posteriors done (main stream) / early draws done (stream2)
    hipEvent_t ev_noise = nullptr;                          // normals of the next draws generated (stream2)
    // pooled pair log-determinants launched ahead (dpmm_step_master_device): list in device memory, records in a pinned block of their own
    hipEvent_t ev_pairs = nullptr;
    DevBuf<int32_t> d_apairs;                               // [2 cap] slot pairs of the launch-ahead job
    size_t apairs_cap = 0;
    std::vector<int32_t> apairs_shadow;
    PinBuf<int32_t> h_apairs_list[2]; int apairs_pin_flip = 0; const int32_t *apairs_pinned_cur = nullptr;      // the fused pair jobs' list in pinned memory (DPMM_OPT_CHAIN_FUSION bit 4)
    PinBuf<double> h_apairs;                                // pinned [cap][DPMM_MASTER_NSCALARS]
    bool apairs_inflight = false, apairs_valid = false;     // main stream has not waited for ev_pairs yet / the records answer dpmm_niw_master_pairs
    std::unordered_map<uint32_t, int> apairs_index;         // (slot_i << 16 | slot_j) -> record
    std::vector<uint8_t> apairs_dirty;                      // [slot] statistics of the slot changed since the job was launched
    std::vector<int32_t> apairs_req;                        // request of dpmm_niw_master_pairs_ahead, consumed by the next dpmm_step_master_device
    PinBuf<char> h_draw;                                    // pinned: lr [K][2] | w [K] of dpmm_niw_master_draw
    bool handover_inflight = false;                         // a hand-over kernel (reads lr / w from h_pin) was launched and the host has not waited behind it
    bool noise_pending = false;                             // dpmm_niw_master_draw asked for the next normals; launched behind the sweep (noise_flush)
    uint32_t noise_pend_epoch = 0;
    int noise_pend_nmat = 0;
    bool noise_inflight = false, noise_valid = false;       // main stream has not waited for ev_noise yet / d_Y[noise_buf] holds the normals of noise_epoch
    uint32_t noise_epoch = 0;
    int noise_nmat = 0, noise_buf = 0;
    bool spec_inflight = false, spec_valid = false;         // main stream has not waited for ev_spec yet / the early draws are still the ones a draw call would make
    uint32_t spec_epoch = 0;
    std::vector<int32_t> spec_slots;
    // index lists of the master kernels (jobs, slot maps) live in device memory and are re-sent only when they change: read from pinned
    // host memory they cost every workgroup a PCIe round trip (~2 us) before its first useful instruction
    DevBuf<int32_t> d_jobs, d_dslots;                        // [2 MAX] jobs of the posterior kernels (main stream) / [MAX] slot map of the draws
    PinBuf<int32_t> h_list[4];                                   // pinned staging ring of device_list
    int h_list_next = 0;
    std::vector<int32_t> jobs_shadow, dslots_shadow;
    PinBuf<uint8_t> h_master;                      // pinned: jobs | slot map | lr | w | small
    bool draws_on_device = false;
    DevBuf<unsigned long long> d_work;   // [DPMM_WORK_SLOTS + 4 DPMM_WORK_PER_WAVE sweep_grid_max]: tile queue heads [4], [8 + 16 q]; [DPMM_WORK_SLOTS + DPMM_WORK_PER_WAVE w ..] executed-work counters of wave w of the last sweep
    int work_waves = 0;                      // most waves of a counted sweep launch since the counters were read
    long long work_launches = 0;             // counted sweep launches since the counters were read
    // options (dpmm_set_option)
    float opt_margin = 50.f;
    int opt_prio = 1;
    int opt_queue_rounds = -1;
    int opt_ball = 1;
    // direction screen of the D in 33..64 sweep (direction_far, niw_sweep.hip; DPMM_OPT_DIRECTION_SCREEN): tables per parameter set, built only while
    // the sweeps report tiles with many candidates (h_need: one word per wave of the last sweep, written by the kernel into pinned memory)
    DevBuf<uint32_t> d_sp_frag;
    DevBuf<uint32_t> d_refb_big;    // D = 128, 256: bf16 images of the cluster-level factors (reference bracket of the LDS-staged kernels), per parameter set
    bool have_refb_big = false;
    DevBuf<uint32_t> d_brk_flag;    // [tiles of 128 points] 1 + k0 where the tile is label-homogeneous, else 0 (niw_bracket_big_kernel)
    DevBuf<float> d_brk_aref;       // [positions of the visiting order] the bracket's lower end of a_k0
    DevBuf<float> d_sp_cons;
    PinBuf<uint32_t> h_need;
    int opt_direction = -1;             // -1: by the previous sweep's candidate counts, 0: never, 1: always
    bool sp_ready = false, sp_regime = false;
    unsigned sp_count = 0;             // parameter sets since the screen came on: every 32nd sweep measures (tail pairs first), the others run it first
    bool sp_last = false;              // the last sweep ran the DIR kernel (its yield words are valid)
    int sp_K = -1;                     // number of clusters of the last parameter set the tables were built for
    int sp_cooldown = 0;               // parameter sets the screen stays off after it removed less than a quarter of what it was given
    int opt_b3 = 1;                    // DPMM_OPT_B3_SUBLABELS: D in 33..64: sub-cluster evaluations through three-plane bf16 images, in kernels of their own (niw_lean.hip)
    bool have_b3 = false;              // the images behind the bracket's in d_tail belong to the parameter set on the device
    int opt_chain = 0x7fffffff & ~(8 | 32);  // (bits 8 / 32: built, value-neutral, measured -- no gain at either size: off by default) DPMM_OPT_CHAIN_FUSION (bit mask): 1 = the sort's starts inside the scatter launch; 2 = the three-plane images in the hand-over launch; 4 = the fused pair jobs' list read from pinned memory; 8 = the bad-cluster reset counted ahead by the histogram and applied by the scatter (no reset launch); 16 = the draws' normals generated inside the posteriors' launch
    DevBuf<uint8_t> d_cert_rec;        // dpmm_debug_norm_cert_points: a byte per point, set by niw_lean_kernel for the tiles its norm certificate settled (empty: no record)
    int opt_lean_norm_cert = 1;        // DPMM_OPT_LEAN_NORM_CERT: niw_lean_kernel settles a tile by the norm bound of a_k0 + the pair-ball test where that suffices (no bracket)
    int opt_pair_ball = 1;             // DPMM_OPT_PAIR_BALL: the lean kernel's full-dimension ball test on the K x K table of pair distances (niw_pair_ball_kernel, K <= 256)
    bool have_pb = false;              // ... and that table belongs to the parameter set on the device
    int opt_lean_dir = 1;              // DPMM_OPT_LEAN_DIRECTION: the lean kernel runs the direction screen while its tables exist (0: no lean launch in that regime, as in rounds 4-5)
    int opt_master_poll = 1;           // DPMM_OPT_MASTER_POLL: dpmm_step_master_device waits on the posteriors' own records in pinned memory (no event between posteriors and draws)
    int opt_lean = 1;                  // DPMM_OPT_LEAN_TILES: tiles the cheap screens settle completely in niw_lean_kernel (-1 automatic is 1 with a regime switch; 0 never)
    DevBuf<uint32_t> d_hard;        // two lists of [2 + ceil(n / 64)] words, taking turns (hard_flip): count | wave tiles the lean kernel left to the general path;
                                       // a lean launch clears the OTHER list's count for its successor (no fill launch), niw_sub_kernel reports the count to h_hard (no copy launch)
    int hard_flip = 0;
    int perm_nbins = 0;                // bins of the sort that wrote sb.perm / sb.bin_start (0: none yet): the lean kernel aligns its tiles to them
    PinBuf<uint32_t> h_hard;        // pinned: the count of the LAST sweep's list (read by the next sweep's regime decision, never waited for)
    bool sn2_tight = false;            // the pair-ball table on the device has the tight sn2 block (else sn2 = sn)
    bool cert_fb = false;              // the last lean launch ran the norm certificate and reported its settled tiles (h_need)
    int cert_cool = 0;                 // parameter sets left without the tight block (the certificate settled too few tiles to pay for it)
    int lean_off = 0;                  // sweeps left without the lean kernel (a sweep that left more than 30 % of its tiles switches it off for lean_backoff)
    bool lean_ran = false;             // the last sweep ran the lean kernel: h_hard holds its list's length
    int lean_backoff = 15;             // 15, doubled by every retry that fails again (up to 1023), back to 15 by one that succeeds: a retry on overlapping
                                       // clusters costs three sweeps' time (MixtureVar 4: 5.3 ms against 1.8), one in 16 was 0.22 ms per step
    int opt_bf16scr = 1;               // D <= 64 sweep: bf16 screens in front of the Float32 16-row screen / of a survivor's first row block (DPMM_OPT_BF16_SCREENS)
    int opt_bracket = 1;               // D <= 64 sweep: certified bf16 bracket of the reference cluster's value instead of its Float32 evaluation where that decides nothing (DPMM_OPT_REF_BRACKET)
    int opt_timing = 0;                // bit 0 / 1 / 2: HIP events around the sweep kernel / the statistics pass / the all-reduces (dpmm_last_kernel_ms, dpmm_last_comm_ms)
    int opt_tail = 1, opt_prescreen = -1, opt_ordered = 1, opt_force_f32 = 0, opt_trace = 0, opt_ref_const = 0;
    int64_t opt_stats_items = 0;
    int opt_stats_groups = 0;
    // collective (dpmm_comm_init: RCCL on the ctx stream; dpmm_comm_init_host: a caller-supplied host all-reduce)
    void *comm = nullptr;
    int rank = 0, world = 1;
    dpmm_host_allreduce_fn host_fn = nullptr;
    void *host_user = nullptr;
    PinBuf<char> h_red;             // pinned staging of the host transport
    hipEvent_t ev_comm[4] = {nullptr, nullptr, nullptr, nullptr};   // [0,1] around the occupancy all-reduce, [2,3] around the packed rows
    bool have_comm_ev[2] = {false, false};
    int64_t comm_bytes[2] = {0, 0};    // payload of the last all-reduce of each kind
    int64_t comm_calls = 0;            // all-reduces since the communicator was attached
    // Bounded waits behind a collective (RCCL transport; DPMM_OPT_COMM_TIMEOUT_MS): a rank that dies between two all-reduces leaves the
    // others inside an RCCL kernel that never ends -- and the reference has the same flaw (its master waits on `fetch`).
    // A watchdog thread per communicator measures how long the host has been blocked on the ctx stream BEHIND AN ENQUEUED COLLECTIVE
    // (`coll_pending`: set when an all-reduce is enqueued, cleared when a wait for the whole stream has returned -- waits on a stream that
    // holds no collective, e.g. an upload or a checkpoint, are never timed); past the deadline it aborts the communicator (ncclCommAbort:
    // the kernel returns), the blocked call comes back and fails with DPMM_ECOMM -- on every surviving rank -- instead of hanging until
    // somebody kills the job.  A peer that is merely SLOW (a long host-side pause between two steps) looks the same from here as one that
    // is gone, and the reference would simply wait: the default limit is therefore half an hour, far beyond any pause of a healthy job.
    // `wd_wait_since` is written, and the abort performed, under `wd_mu`: the host thread that comes back from its wait either clears the
    // mark before the watchdog looks, or finds the communicator aborted -- it never enqueues on a communicator that is being aborted.
    // After an abort only the collectives refuse (DPMM_ECOMM); entry points that use none (dpmm_get_labels, dpmm_sync) keep working, so
    // that the state can still be saved.  The host transport's callback owns its own time-out.
    int comm_timeout_ms = 1800000;
    bool coll_pending = false;         // an RCCL collective was enqueued and no full wait on the ctx stream has returned since
    bool abort_reported = false;       // the call that was blocked when the watchdog fired has returned DPMM_ECOMM
    std::thread *watchdog = nullptr;
    std::mutex wd_mu;
    std::condition_variable wd_cv;
    bool wd_stop = false;
    std::atomic<int64_t> wd_wait_since{0};      // steady-clock ms when the host began to block on the stream; 0: not blocked
    std::atomic<bool> comm_aborted{false};
    // ONE collective per per-step pass (DPMM_OPT_ONE_COLLECTIVE; NIW, communicator attached): see run_stats
    int opt_one_collective = -1;       // -1: automatic (rows short enough that half a message more is cheaper than a second collective), 0 / 1
    DevBuf<uint8_t> d_cside;        // [DPMM_MAX_CLUSTERS] clusters whose sub-labels this shard reset speculatively: the side its points were on (1 / 2), 0: none
    DevBuf<double> d_red;           // [3 Kcap][packed_stride]: what travels -- 2K rows of the labels as swept | K re-drawn left rows -- input of the finalize kernel
    bool last_pass_one_collective = false;
    bool undo_pending = false;         // niw_undo_reset_kernel of the last one-collective pass not launched yet (flush_undo)

    std::string err;
};

static inline double now_ms() {
    timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}
#define HIPCHK(ctx, expr)                                                                               \
    do {                                                                                                \
        const double t0__ = (ctx)->opt_trace ? now_ms() : 0.0;                                          \
        hipError_t e__ = (expr);                                                                        \
        if ((ctx)->opt_trace) {                                                                           \
            const double dt__ = now_ms() - t0__;                                                        \
            if (dt__ > 5.0) fprintf(stderr, "[dpmm slow] %.2f ms in %s (line %d)\n", dt__, #expr, __LINE__); \
        }                                                                                               \
        if (e__ == hipErrorLaunchTimeOut && (ctx)->comm_aborted.load(std::memory_order_relaxed)) {      /* (sync_stream / sync_event: the watchdog fired during this wait) */ \
            (ctx)->err = "collective timed out: a peer rank is gone or stuck (communicator aborted after DPMM_OPT_COMM_TIMEOUT_MS)"; \
            return DPMM_ECOMM;                                                                          \
        }                                                                                               \
        if (e__ != hipSuccess) {                                                                        \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e__);                            \
            return DPMM_EHIP;                                                                           \
        }                                                                                               \
    } while (0)

static inline int64_t steady_ms() {
    return std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// Blocking waits on the ctx stream go through these two: with an RCCL communicator attached the watchdog sees how long they last.
static inline void wd_arm(dpmm_ctx *c) {
    std::lock_guard<std::mutex> lk(c->wd_mu);
    c->wd_wait_since.store(steady_ms() | 1, std::memory_order_relaxed);
}
// true: the watchdog aborted the communicator while this wait was armed (reported once, by the call that was blocked)
static inline bool wd_disarm(dpmm_ctx *c) {
    std::lock_guard<std::mutex> lk(c->wd_mu);      // (an abort in progress finishes first: the caller then sees it)
    c->wd_wait_since.store(0, std::memory_order_relaxed);
    if (c->comm_aborted.load() && !c->abort_reported) { c->abort_reported = true; return true; }
    return false;
}
static inline hipError_t sync_stream(dpmm_ctx *c, hipStream_t st) {
    if (st == c->stream) c->sync_gen += 1;        // (everything queued on the main stream so far has run when this returns)
    if (!c->watchdog || !c->coll_pending) return hipStreamSynchronize(st);
    wd_arm(c);
    hipError_t e = hipStreamSynchronize(st);
    if (wd_disarm(c)) e = hipErrorLaunchTimeOut;
    else if (e == hipSuccess && st == c->stream) c->coll_pending = false;      // the stream is empty: no collective left on it
    return e;
}
static inline hipError_t sync_event(dpmm_ctx *c, hipEvent_t ev) {
    if (!c->watchdog || !c->coll_pending) return hipEventSynchronize(ev);
    wd_arm(c);
    hipError_t e = hipEventSynchronize(ev);
    if (wd_disarm(c)) e = hipErrorLaunchTimeOut;
    return e;
}

static int fail(dpmm_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

// The one grow-on-demand routine of this file.  grow: a buffer that holds `need` bytes is left alone (a compare and a return: it sits on
// the per-step path); otherwise the ctx stream is waited for -- something queued may still read the old block -- and the buffer replaced
// (contents are not kept).  floor == 0: exactly `need` bytes; else the smallest floor * 2^k that holds them.  regrow is the second half
// alone, for the callers that wait for more than the ctx stream, or on purpose for nothing, before they let go of the old block.
template <class Buf>
static int regrow(dpmm_ctx *c, Buf &buf, size_t need, const char *who, const char *what, size_t floor = 0) {
    const size_t cap = grow_capacity(need, floor);
    if (buf.alloc(cap) != hipSuccess)
        return fail(c, DPMM_EHIP, std::string(who) + ": out of device memory for the " + what + " (" + std::to_string((unsigned long long)cap) + " bytes)");
    return DPMM_OK;
}
template <class Buf>
static inline int grow(dpmm_ctx *c, Buf &buf, size_t need, const char *who, const char *what, size_t floor = 0) {
    if (need <= buf.bytes) return DPMM_OK;
    HIPCHK(c, sync_stream(c, c->stream));
    return regrow(c, buf, need, who, what, floor);
}
// a table of the sampler (include/dpmm_hip_sample.h): exactly `bytes`, filled from the host
template <typename T>
static int sampler_table(dpmm_ctx *c, DevBuf<T> &dst, const T *src, size_t bytes) {
    HIPCHK(c, dst.alloc(bytes));
    HIPCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return DPMM_OK;
}
// pinned host staging of every per-step transfer
static inline int ensure_pinned(dpmm_ctx *c, size_t bytes) { return grow(c, c->h_pin, bytes, "dpmm", "pinned staging block", (size_t)1 << 20); }

// ---- RCCL, bound at run time ---------------------------------------------------------------------------------------------
// The library must load (and `pytest -m "not gpu"` must be able to check its exports) on machines without RCCL, and a
// process that also uses torch.distributed must end up with ONE copy of librccl: the symbols are looked up with dlopen,
// first among the libraries already mapped, then by soname, then under /opt/rocm.
struct UidByValue { char internal[128]; };
namespace {
struct Rccl {
    void *handle = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, /* ncclUniqueId by value */ UidByValue, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*CommAbort)(void *) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    std::string err;
};
}  // namespace
static std::string g_rccl_path;   // dpmm_comm_use_library
static Rccl &rccl() {
    static Rccl r;
    if (r.handle || !r.err.empty()) return r;
    const char *names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so", "/opt/rocm/lib/librccl.so.1"};
    if (!g_rccl_path.empty()) r.handle = dlopen(g_rccl_path.c_str(), RTLD_NOW | RTLD_GLOBAL);
    if (!r.handle) for (const char *n : names) { r.handle = dlopen(n, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL); if (r.handle) break; }
    if (!r.handle) for (const char *n : names) { r.handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (r.handle) break; }
    if (!r.handle) { r.err = std::string("librccl.so not found: ") + (dlerror() ? dlerror() : ""); return r; }
    auto sym = [&](const char *n) { void *p = dlsym(r.handle, n); if (!p && r.err.empty()) r.err = std::string("missing RCCL symbol ") + n; return p; };
    r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(sym("ncclGetUniqueId"));
    r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(sym("ncclCommInitRank"));
    r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(sym("ncclCommDestroy"));
    r.CommAbort = reinterpret_cast<decltype(r.CommAbort)>(dlsym(r.handle, "ncclCommAbort"));      // (optional: the watchdog needs it)
    r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(sym("ncclAllReduce"));
    r.AllGather = reinterpret_cast<decltype(r.AllGather)>(sym("ncclAllGather"));
    r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(sym("ncclGetErrorString"));
    return r;
}
enum { kNcclInt64 = 4, kNcclFloat64 = 8, kNcclInt8 = 0, kNcclSum = 0 };   // ncclDataType_t / ncclRedOp_t values of rccl.h

static inline bool comm_attached(const dpmm_ctx *c) { return c->comm != nullptr || c->host_fn != nullptr; }
// In-place all-reduce(sum) of a device buffer over the ranks, stream-ordered on the ctx stream.  `kind`: 0 = Int64 sub-cluster
// occupancies, 1 = Float64 packed rows (HIP events around each kind: dpmm_last_comm_ms).  Transport: RCCL (dpmm_comm_init) or the
// caller's host function (dpmm_comm_init_host: device -> pinned, synchronise, fn, pinned -> device).
static int comm_allreduce(dpmm_ctx *c, void *dbuf, size_t count, int kind) {
    const bool f64 = kind == 1;
    if (c->opt_timing & 4) {
        if (!c->ev_comm[0]) for (auto &e : c->ev_comm) HIPCHK(c, hipEventCreate(&e));
        HIPCHK(c, hipEventRecord(c->ev_comm[2 * kind], c->stream));
    }
    if (c->comm) {
        Rccl &r = rccl();
        if (c->comm_aborted.load()) return fail(c, DPMM_ECOMM, "the communicator was aborted after a collective timed out: attach a new one (dpmm_comm_release, dpmm_comm_init)");
        const int rc = r.AllReduce(dbuf, dbuf, count, f64 ? kNcclFloat64 : kNcclInt64, kNcclSum, c->comm, c->stream);
        if (rc != 0) return fail(c, DPMM_ECOMM, std::string("ncclAllReduce: ") + r.GetErrorString(rc));
        c->coll_pending = true;
    } else {
        const size_t bytes = count * 8;
        if (int rc = grow(c, c->h_red, bytes, "host all-reduce", "pinned staging block", (size_t)1 << 16)) return rc;
        HIPCHK(c, launch_copy_bytes(c->h_red, dbuf, bytes, c->stream));
        HIPCHK(c, sync_stream(c, c->stream));
        const int rc = c->host_fn(c->host_user, c->h_red, (int64_t)count, f64 ? 1 : 0);
        if (rc != 0) return fail(c, DPMM_ECOMM, "host all-reduce callback failed (code " + std::to_string(rc) + ")");
        HIPCHK(c, launch_copy_bytes(dbuf, c->h_red, bytes, c->stream));
    }
    if (c->opt_timing & 4) HIPCHK(c, hipEventRecord(c->ev_comm[2 * kind + 1], c->stream));
    c->have_comm_ev[kind] = (c->opt_timing & 4) != 0;
    c->comm_bytes[kind] = (int64_t)count * 8;
    ++c->comm_calls;
    return DPMM_OK;
}
static void watchdog_stop(dpmm_ctx *c) {
    if (!c->watchdog) return;
    { std::lock_guard<std::mutex> lk(c->wd_mu); c->wd_stop = true; }
    c->wd_cv.notify_all();
    c->watchdog->join();
    delete c->watchdog;
    c->watchdog = nullptr;
    c->wd_stop = false;
}
static void watchdog_start(dpmm_ctx *c) {
    if (c->watchdog || !rccl().CommAbort) return;
    c->watchdog = new std::thread([c]() {
        std::unique_lock<std::mutex> lk(c->wd_mu);
        while (!c->wd_stop) {
            c->wd_cv.wait_for(lk, std::chrono::milliseconds(20));
            if (c->wd_stop) break;
            const int64_t since = c->wd_wait_since.load(std::memory_order_relaxed);
            const int limit = c->comm_timeout_ms;
            if (since != 0 && limit > 0 && steady_ms() - since > limit && !c->comm_aborted.load()) {
                c->comm_aborted.store(true);
                rccl().CommAbort(c->comm);          // the collective's kernel returns, the blocked host call with it
            }
        }
    });
}
static void comm_release(dpmm_ctx *c) {
    watchdog_stop(c);
    if (c->comm) { if (!c->comm_aborted.load()) rccl().CommDestroy(c->comm); c->comm = nullptr; }      // (ncclCommAbort released an aborted one)
    c->comm_aborted.store(false);
    c->coll_pending = false; c->abort_reported = false;
    c->host_fn = nullptr; c->host_user = nullptr;
    c->world = 1; c->rank = 0;
    c->have_comm_ev[0] = c->have_comm_ev[1] = false;
    c->comm_bytes[0] = c->comm_bytes[1] = 0; c->comm_calls = 0;
}

#pragma GCC visibility push(default)
extern "C" {

int dpmm_abi_version(void) { return DPMM_ABI_VERSION; }

const char *dpmm_last_error(const dpmm_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

// The buffers whose size depends on the number of clusters are about to be re-allocated (ensure_capacity, member by member): what is
// known about their contents goes with them
static void free_params(dpmm_ctx *c) {
    c->mspec_valid = false;
    c->have_refb_big = false;
}

// (re)allocate everything whose size depends on the number of clusters
static int ensure_capacity(dpmm_ctx *c, int K) {
    if (K <= c->Kcap) return DPMM_OK;
    int cap = std::max(8, c->Kcap);
    while (cap < K) cap *= 2;
    cap = std::min(cap, DPMM_MAX_CLUSTERS);
    HIPCHK(c, sync_stream(c, c->stream));
    free_params(c);
    const size_t D = (size_t)c->D;
    if (c->prior == DPMM_PRIOR_NIW) {
        const size_t NP = (size_t)c->NB * (c->NB + 1) / 2;
        HIPCHK(c, c->d_raw.alloc(sizeof(float) * 3 * cap * D * D));
        HIPCHK(c, c->d_mu.alloc(sizeof(float) * 3 * cap * D));
        HIPCHK(c, c->d_Rp.alloc(sizeof(float) * 3 * cap * NP * 256));
        HIPCHK(c, c->d_mup.alloc(sizeof(float) * 3 * cap * 16 * c->NB));
        HIPCHK(c, c->d_lam.alloc(sizeof(float) * cap));
        if (c->NB == 8 || c->NB == 16) HIPCHK(c, c->d_refb_big.alloc(sizeof(uint32_t) * cap * niw_refb_big_words(c->NB)));
        HIPCHK(c, c->d_tail.alloc(sizeof(float) * (c->NB == 4 ? niw_tail_floats(cap) : 16 * (cap + 2) + 16 * cap + (size_t)REFB_WORDS * cap)));      // pair records | per-cluster ball records | bf16 images of the reference bracket | (NB = 4) three-plane images + offsets of niw_lean.hip
        HIPCHK(c, c->d_mdist.alloc(sizeof(float) * (size_t)cap * cap));
    } else {
        const size_t NT = (size_t)(c->ldx + 15) / 16, NRB = (size_t)(3 * cap + 15) / 16;
        const size_t lp16 = sizeof(uint32_t) * std::max(mult_pack_bf16_words(3 * cap, c->ldx), mult_pack_u8_words(3 * cap, (c->D + 127) / 128 * 128));
        HIPCHK(c, c->d_raw.alloc(sizeof(float) * 3 * cap * (size_t)c->ldx));
        HIPCHK(c, c->d_Rp.alloc(sizeof(float) * NRB * NT * 256));
        HIPCHK(c, c->d_Lp16.alloc(lp16));
        HIPCHK(c, c->d_raw2.alloc(sizeof(float) * 3 * cap * (size_t)c->ldx));
        HIPCHK(c, c->d_Rp2.alloc(sizeof(float) * NRB * NT * 256));
        HIPCHK(c, c->d_Lp16_2.alloc(lp16));
    }
    HIPCHK(c, c->d_cst.alloc(sizeof(float) * 3 * cap));
    HIPCHK(c, c->d_tdf.alloc(sizeof(float) * 6 * cap));
    // sweep scratch: one a_k row set per resident workgroup; the Multinomial kernel keeps all 3K rows
    const int rows = (c->prior == DPMM_PRIOR_NIW) ? cap : 3 * cap;
    c->scratch_stride = (int64_t)c->sweep_grid * c->tile;
    HIPCHK(c, c->d_scratch.alloc(sizeof(float) * (size_t)rows * (size_t)c->scratch_stride));
    // statistics
    c->max_items = (int)((c->n + c->chunk - 1) / c->chunk) + 2 * cap;
    // NIW: one slab per SLOT (a workgroup of the statistics kernel, or a bin whose first item lies inside a workgroup's range); Multinomial: per item
    const size_t nslabs = c->prior == DPMM_PRIOR_NIW ? (size_t)NIW_STATS_MAX_GROUPS + 2 * (size_t)cap : (size_t)c->max_items;
    HIPCHK(c, c->d_slabs.alloc(sizeof(double) * nslabs * (size_t)c->slab_stride));
    HIPCHK(c, c->d_out.alloc(sizeof(double) * 2 * cap * (size_t)c->packed_stride + DPMM_MAX_CLUSTERS + 64));   // rows | bad-cluster flags
    HIPCHK(c, c->d_red.alloc(sizeof(double) * 3 * (size_t)cap * (size_t)c->packed_stride));
    HIPCHK(c, c->d_ccache.alloc(sizeof(double) * cap * (size_t)c->packed_stride));
    HIPCHK(c, hipMemsetAsync(c->d_ccache, 0, sizeof(double) * cap * (size_t)c->packed_stride, c->stream));      // (on the stream its readers run on)
    c->cache_force = true;
    c->Kcap = cap;
    return DPMM_OK;
}

// words of ONE tile list of the lean sweep: count + (position, count) per tile; at most ceil(n / 64) + NIW_LEAN_MAX_BINS tiles (bin-aligned)
static size_t hard_list_words(int64_t n) { return 4 + 2 * ((size_t)((n + 63) / 64) + NIW_LEAN_MAX_BINS + 2); }

// the kernels' view of the sort buffers (dpmm_kernels.h SortBufs): the owners are c->sort_mem
static void sort_view(dpmm_ctx *c) {
    auto &m = c->sort_mem;
    SortBufs &b = c->sb;
    b.tile_hist = m.tile_hist; b.tile_cnt = m.tile_cnt; b.spec_bins = m.spec_bins; b.tile_spec = m.tile_spec; b.fast_total = m.fast_total;
    b.ticket = m.ticket; b.prev_lab = m.prev_lab; b.cdirty = m.cdirty; b.cmode = m.cmode; b.bin_total = m.bin_total; b.bin_start = m.bin_start;
    b.perm = m.perm; b.item_start = m.item_start; b.bin_sel = m.bin_sel; b.perm_total = m.perm_total;
}

int dpmm_create(dpmm_ctx **out, int prior_kind, int D, int64_t n_local, int64_t first_index, int device, uint64_t seed) {
    if (!out) return fail(nullptr, DPMM_EINVAL, "ctx out pointer is null");
    *out = nullptr;
    if (prior_kind != DPMM_PRIOR_NIW && prior_kind != DPMM_PRIOR_MULT) return fail(nullptr, DPMM_EINVAL, "unknown prior kind");
    if (D < 1 || n_local < 0 || first_index < 0) return fail(nullptr, DPMM_EINVAL, "bad D / n_local / first_index");
    if (n_local > 2000000000LL) return fail(nullptr, DPMM_ELIMIT, "n_local exceeds the Int32 point index of this build");
    if (prior_kind == DPMM_PRIOR_NIW && D > DPMM_MAX_DIM_NIW) return fail(nullptr, DPMM_ELIMIT, "NIW: D > DPMM_MAX_DIM_NIW");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, DPMM_ENODEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(nullptr, DPMM_ENODEVICE, "device ordinal out of range");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, DPMM_ENODEVICE, "hipSetDevice failed");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(nullptr, DPMM_ENODEVICE, "hipGetDeviceProperties failed");
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(nullptr, DPMM_ENODEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");

    dpmm_ctx *c = new dpmm_ctx();
    c->prior = prior_kind; c->D = D; c->n = n_local; c->first = first_index; c->device = device; c->seed = seed;
    c->ldx = (D + 3) / 4 * 4;
    // Multinomial rows are streamed in 128-byte pieces per point: pad the row to a multiple of 32 floats so that no piece straddles
    // two cache lines (D = 1000: rows of 4000 B made every piece touch two lines, HBM reads 1.2-1.3 x the algorithmic bytes)
    if (prior_kind == DPMM_PRIOR_MULT && D >= 32) c->ldx = (D + 31) / 32 * 32;
    c->cus = prop.multiProcessorCount;
    auto bail = [&](int code) { std::string m = c->err; dpmm_destroy(c); g_create_error = m; return code; };
#define CHK_CREATE(expr)                                                                  \
    do {                                                                                  \
        hipError_t e__ = (expr);                                                          \
        if (e__ != hipSuccess) { c->err = std::string(#expr) + ": " + hipGetErrorString(e__); return bail(DPMM_EHIP); } \
    } while (0)
    CHK_CREATE(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (auto &e : c->ev) CHK_CREATE(hipEventCreate(&e));
    if (prior_kind == DPMM_PRIOR_NIW) {
        c->NB = nb_for_dim(D);
        c->tile = niw_tile_points(c->NB);
        c->slab_stride = niw_slab_stride(D);
        c->packed_stride = 1 + (int64_t)D + (int64_t)D * (D + 1) / 2;
        c->sweep_grid = c->cus * niw_occupancy(c->NB);
        CHK_CREATE(c->d_row_off.alloc(sizeof(int32_t) * (size_t)c->packed_stride));
        CHK_CREATE(c->d_inv_off.alloc(sizeof(int32_t) * (size_t)c->slab_stride));
        CHK_CREATE(launch_niw_row_offsets(c->d_row_off, c->d_inv_off, D, c->packed_stride, c->stream));
    } else {
        c->tile = mult_tile_points();
        c->slab_stride = mult_slab_stride(D);
        c->packed_stride = 1 + (int64_t)D;
        c->sweep_grid = c->cus * 2;
    }
    c->ntiles = (n_local + c->tile - 1) / c->tile;
    if (c->ntiles < c->sweep_grid) c->sweep_grid = (int)std::max<int64_t>(1, c->ntiles);
    c->sweep_grid_max = c->sweep_grid;
    // statistics work items: ~4 per resident wave slot (2 waves/SIMD) so the last round is not mostly empty
    // work items of the statistics pass: the NIW kernel hands every workgroup a contiguous RANGE of items, so finer items
    // only improve the balance (ceil(items / groups) granularity) -- 16384 at D <= 64 (1.05 -> 0.85 ms at N = 1e7); slabs
    // are allocated per item, which is why the large-D kernels (280 KB per slab at D = 256) stay at 8192
    const int64_t target_items = (c->prior == DPMM_PRIOR_NIW && c->D <= 64) ? 16384 : 8192;
    // NIW: the statistics kernel balances its workgroups' ranges to ONE item and slabs are per slot, not per item -- items only set the
    // granularity of the balance: 32 points (8 k-steps) for the one-wave D <= 64 kernels, 256 for the multi-panel kernels (16-point batches).
    // Multinomial: one workgroup and one slab per item: 8192 items.
    const int64_t min_chunk = (c->prior == DPMM_PRIOR_NIW && c->D <= 64) ? 32 : 256;
    const int64_t target_items2 = (c->prior == DPMM_PRIOR_NIW && c->D <= 64) ? 65536 : target_items;
    c->chunk = (int)std::max<int64_t>(min_chunk, ((n_local + target_items2 - 1) / target_items2 + 3) / 4 * 4);
    c->chunk_dense = c->chunk;
    const size_t nalloc = (size_t)std::max<int64_t>(n_local, 1);
    // (Multinomial: the dense matrix is allocated by the first dense upload -- ensure_points_buffer -- a context that is given sparse points never holds one)
    if (prior_kind == DPMM_PRIOR_NIW) CHK_CREATE(c->dX.alloc(sizeof(float) * nalloc * (size_t)c->ldx));
    CHK_CREATE(c->dbins.alloc(sizeof(int32_t) * nalloc));
    // sort tiles: 512 points per sorting wave below 4e6 points (the tile kernels are one-wave latency chains: at the 8-GPU shard size four
    // times as many waves of a quarter of the trips each), 2048 above; the tables are sized for whichever is in use (DPMM_OPT_SORT_TILE
    // may switch while the shard is small enough for the small tile's tables)
    c->sb.tile = n_local <= 4000000 ? SORT_TILE_SMALL : SORT_TILE;
    const int alloc_tile = c->sb.tile;           // (DPMM_OPT_SORT_TILE re-allocates when it selects the smaller tile: at N = 1e7 the small tile's tables are 320 MB, these 80 MB)
    c->sort_tile_min = alloc_tile;
    c->nt_sort = (int)((n_local + alloc_tile - 1) / alloc_tile);
    const size_t nbmax = 2 * DPMM_MAX_CLUSTERS;
    CHK_CREATE(c->sort_mem.tile_hist.alloc(sizeof(int32_t) * nbmax * (size_t)std::max(1, c->nt_sort)));
    CHK_CREATE(c->sort_mem.tile_cnt.alloc(sizeof(int32_t) * nbmax * (size_t)std::max(1, c->nt_sort)));
    CHK_CREATE(c->sort_mem.tile_spec.alloc(sizeof(int32_t) * (size_t)STEP_SPEC_MAX_BINS * (size_t)std::max(1, c->nt_sort)));
    CHK_CREATE(c->sort_mem.spec_bins.alloc(sizeof(int32_t) * nalloc));
    CHK_CREATE(c->sort_mem.fast_total.alloc(sizeof(int32_t) * nbmax * FAST_TOTAL_STRIDE));
    CHK_CREATE(hipMemsetAsync(c->sort_mem.fast_total, 0, sizeof(int32_t) * nbmax * FAST_TOTAL_STRIDE, c->stream));
    CHK_CREATE(c->sort_mem.ticket.alloc(sizeof(unsigned)));
    CHK_CREATE(hipMemsetAsync(c->sort_mem.ticket, 0, sizeof(unsigned), c->stream));
    CHK_CREATE(c->sort_mem.prev_lab.alloc(sizeof(uint16_t) * (((size_t)nalloc + SORT_TILE - 1) / SORT_TILE * SORT_TILE)));
    CHK_CREATE(hipMemsetAsync(c->sort_mem.prev_lab, 0xFF, sizeof(uint16_t) * (((size_t)nalloc + SORT_TILE - 1) / SORT_TILE * SORT_TILE), c->stream));
    CHK_CREATE(c->sort_mem.cdirty.alloc(DPMM_MAX_CLUSTERS + 8));
    CHK_CREATE(hipMemsetAsync(c->sort_mem.cdirty, 1, DPMM_MAX_CLUSTERS + 8, c->stream));
    CHK_CREATE(c->sort_mem.cmode.alloc(DPMM_MAX_CLUSTERS));
    CHK_CREATE(hipMemsetAsync(c->sort_mem.cmode, 0, DPMM_MAX_CLUSTERS, c->stream));
    CHK_CREATE(c->sort_mem.bin_total.alloc(sizeof(int32_t) * nbmax));
    CHK_CREATE(c->sort_mem.bin_start.alloc(sizeof(int32_t) * (nbmax + 1)));
    CHK_CREATE(c->sort_mem.item_start.alloc(sizeof(int32_t) * (nbmax + 1)));
    CHK_CREATE(c->sort_mem.perm.alloc(sizeof(int32_t) * nalloc));
    CHK_CREATE(c->sort_mem.bin_sel.alloc(nbmax));
    c->sel_capacity = (int)nbmax;
    CHK_CREATE(c->sort_mem.perm_total.alloc(sizeof(int32_t)));
    sort_view(c);
    CHK_CREATE(c->d_small.alloc(sizeof(int32_t) * 4 * DPMM_MAX_CLUSTERS));
    CHK_CREATE(c->d_counts64.alloc(sizeof(long long) * 2 * DPMM_MAX_CLUSTERS));
    CHK_CREATE(c->d_cside.alloc(DPMM_MAX_CLUSTERS));
    CHK_CREATE(hipMemsetAsync(c->d_cside, 0, DPMM_MAX_CLUSTERS, c->stream));
    if (c->prior == DPMM_PRIOR_NIW && c->NB == 4) {
        CHK_CREATE(c->d_sp_frag.alloc(sizeof(uint32_t) * (size_t)SP_MAXK * SP_FRAG_WORDS));
        CHK_CREATE(c->d_sp_cons.alloc(sizeof(float) * (size_t)SP_MAXK * SP_CONS_FLOATS));
        // (20 g words in three parts: need_lean_settled, need_lean_dir)
        CHK_CREATE(c->h_need.alloc(sizeof(uint32_t) * 20 * (size_t)std::max(1, c->sweep_grid_max)));
        memset(c->h_need, 0, sizeof(uint32_t) * 20 * (size_t)std::max(1, c->sweep_grid_max));
        if (c->NB == 4) {
            const size_t hw = hard_list_words(n_local);
            CHK_CREATE(c->d_hard.alloc(sizeof(uint32_t) * 2 * hw));
            CHK_CREATE(hipMemsetAsync(c->d_hard, 0, sizeof(uint32_t) * 2 * hw, c->stream));
            CHK_CREATE(c->h_hard.alloc(64));
            memset(c->h_hard, 0, 64);
        }
    }
    CHK_CREATE(c->d_work.alloc(sizeof(unsigned long long) * (DPMM_WORK_SLOTS + 4 * DPMM_WORK_PER_WAVE * (size_t)std::max(1, c->sweep_grid_max))));
    CHK_CREATE(hipMemsetAsync(c->d_work, 0, sizeof(unsigned long long) * (DPMM_WORK_SLOTS + 4 * DPMM_WORK_PER_WAVE * (size_t)std::max(1, c->sweep_grid_max)), c->stream));
#undef CHK_CREATE
    *out = c;
    return DPMM_OK;
}

int dpmm_destroy(dpmm_ctx *c) {
    if (!c) return DPMM_OK;
    hipSetDevice(c->device);
    if (c->stream && !c->comm_aborted.load()) hipStreamSynchronize(c->stream);
    if (c->stream2) hipStreamSynchronize(c->stream2);
    comm_release(c);
    for (auto &e : c->ev_part) if (e) hipEventDestroy(e);
    for (hipEvent_t e : {c->ev_master, c->ev_spec, c->ev_noise, c->ev_pairs, c->ev_rows}) if (e) hipEventDestroy(e);
    for (auto &e : c->ev_comm) if (e) hipEventDestroy(e);
    for (auto &e : c->ev) if (e) hipEventDestroy(e);
    if (c->stream2) hipStreamDestroy(c->stream2);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;       // every buffer is a member: freed here, behind both streams
    return DPMM_OK;
}

// after the points are in place: the Multinomial fast path needs to know whether every count is exact in bf16
static int finish_upload(dpmm_ctx *c) {
    if (c->prior == DPMM_PRIOR_MULT) {
        const bool force_f32 = c->opt_force_f32 != 0;
        const int was_u8 = c->x_u8, was_bf16 = c->x_bf16_exact;
        int *flag = reinterpret_cast<int *>(c->d_small.get());
        HIPCHK(c, hipMemsetAsync(flag, 0, sizeof(int), c->stream));
        HIPCHK(c, launch_bf16_exact_check(c->dX, c->n * c->ldx, flag, c->stream));
        int h = 1;
        HIPCHK(c, hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, sync_stream(c, c->stream));
        c->x_bf16_exact = (h == 0 && !force_f32) ? 1 : 0;
        c->x_u8 = 0;
        if (c->x_bf16_exact && !c->opt_no_u8 && c->n > 0) {
            // small non-negative integers (bag-of-words counts): keep a lossless byte copy and stream 1 byte per element
            c->ld8 = (c->D + 127) / 128 * 128;
            if (!c->dX8) HIPCHK(c, c->dX8.alloc((size_t)c->n * (size_t)c->ld8));
            HIPCHK(c, hipMemsetAsync(flag, 0, sizeof(int), c->stream));
            HIPCHK(c, launch_u8_convert(c->dX, c->ldx, c->D, c->n, c->dX8, c->ld8, flag, c->stream));
            HIPCHK(c, hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, sync_stream(c, c->stream));
            c->x_u8 = (h == 0) ? 1 : 0;
            if (!c->x_u8) c->dX8.reset();
            // every Multinomial kernel of a byte-path context reads the byte copy (a lossless re-encoding): the Float32 matrix (4 bytes per
            // element, 4 GB at D = 1000, N = 1e6) is dead weight from here on; a new upload allocates it again
            else c->dX.reset();
        }
        // parameters that stay in place across the upload were packed for the OLD points' sweep kernel (byte planes / bf16 planes / Float32
        // fragments): when the new points take another kernel, the images it reads are made from the raw rows now
        if (c->have_params && c->d_raw && (was_u8 != c->x_u8 || was_bf16 != c->x_bf16_exact || c->repack_pending)) {
            HIPCHK(c, launch_mult_pack(c->d_raw, c->d_Rp, 3 * c->K, c->ldx, c->stream));
            c->rp_current = true;
            if (c->x_u8) HIPCHK(c, launch_mult_pack_u8(c->d_raw, c->d_Lp16, 3 * c->K, c->ldx, c->ld8, c->stream));
            else if (c->x_bf16_exact) HIPCHK(c, launch_mult_pack_bf16(c->d_raw, c->d_Lp16, 3 * c->K, c->ldx, c->stream));
            c->mspec_valid = false;
        }
        c->repack_pending = false;
    }
    HIPCHK(c, sync_stream(c, c->stream));
    // new points: the cached cluster-level statistics (derive_rows_kernel) and the rows a device master would draw from belong to the old ones
    c->cache_force = true;
    c->rows_full_K = -1;
    return DPMM_OK;
}

// Points per statistics item for the kind of points in force.  Dense: as ever.  Sparse: a slab is D doubles in global memory (512 KB at
// D = 65536), so the items that cover the points are sized to keep their slabs within 256 MB (at least 64 items; never finer than the dense
// items: unchanged up to D = 4096).  The 2 Kcap slabs for the bins' ragged ends come on top, whatever the chunk.
static int set_points_chunk(dpmm_ctx *c, bool sparse) {
    int want = c->chunk_dense;
    if (sparse) {
        const int64_t items = std::max<int64_t>(64, std::min<int64_t>(8192, ((int64_t)256 << 20) / (8 * (int64_t)c->D)));
        want = std::max(want, (int)std::max<int64_t>(256, ((c->n + items - 1) / items + 3) / 4 * 4));
    }
    if (want == c->chunk) return DPMM_OK;
    HIPCHK(c, sync_stream(c, c->stream));
    c->chunk = want;
    if (c->Kcap > 0) {      // the slabs are allocated per item (ensure_capacity)
        c->max_items = (int)((c->n + c->chunk - 1) / c->chunk) + 2 * c->Kcap;
        HIPCHK(c, c->d_slabs.alloc(sizeof(double) * (size_t)c->max_items * (size_t)c->slab_stride));
    }
    return DPMM_OK;
}
static void free_sparse_points(dpmm_ctx *c) {
    c->d_cp.reset(); c->d_ri.reset(); c->d_val.reset(); c->nnz = 0;
}
static int ensure_points_buffer(dpmm_ctx *c) {       // (a byte-path Multinomial context gave its Float32 matrix back; one with sparse points never had it)
    if (c->x_sparse) {
        HIPCHK(c, sync_stream(c, c->stream));
        free_sparse_points(c);
        c->x_sparse = 0;
        c->repack_pending = true;
        if (int rc = set_points_chunk(c, false)) return rc;
    }
    if (!c->dX) HIPCHK(c, c->dX.alloc(sizeof(float) * (size_t)std::max<int64_t>(c->n, 1) * (size_t)c->ldx));
    return DPMM_OK;
}
static int upload_common(dpmm_ctx *c, const float *X, int64_t ldx, hipMemcpyKind kind) {
    if (!c) return DPMM_EINVAL;
    if (!X && c->n > 0) return fail(c, DPMM_EINVAL, "X is null");
    if (ldx < c->D) return fail(c, DPMM_EINVAL, "ldx < D");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_points_buffer(c)) return rc;
    if (c->n > 0) {
        if (c->ldx != c->D) HIPCHK(c, hipMemsetAsync(c->dX, 0, sizeof(float) * (size_t)c->n * c->ldx, c->stream));
        HIPCHK(c, hipMemcpy2DAsync(c->dX, sizeof(float) * c->ldx, X, sizeof(float) * ldx, sizeof(float) * c->D, (size_t)c->n, kind, c->stream));
        if (int rc = finish_upload(c)) return rc;
    }
    c->have_points = true;
    c->cache_force = true;          // (also for n == 0; finish_upload does it for every path that moved points)
    c->rows_full_K = -1;
    return DPMM_OK;
}

int dpmm_upload_points(dpmm_ctx *c, const float *X, int64_t ldx) { return upload_common(c, X, ldx, hipMemcpyHostToDevice); }
int dpmm_upload_points_device(dpmm_ctx *c, const float *dX, int64_t ldx) { return upload_common(c, dX, ldx, hipMemcpyDeviceToDevice); }

int dpmm_upload_points_npy(dpmm_ctx *c, const void *rows, int is_f64, int64_t ld, int nan_to_zero) {
    if (!c) return DPMM_EINVAL;
    if (!rows && c->n > 0) return fail(c, DPMM_EINVAL, "rows is null");
    if (ld < c->D) return fail(c, DPMM_EINVAL, "ld < D");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_points_buffer(c)) return rc;
    if (c->n > 0) {
        if (c->ldx != c->D) HIPCHK(c, hipMemsetAsync(c->dX, 0, sizeof(float) * (size_t)c->n * c->ldx, c->stream));
        const size_t esz = is_f64 ? sizeof(double) : sizeof(float);
        const int64_t chunk_rows = std::max<int64_t>(1, std::min<int64_t>(c->n, ((int64_t)128 << 20) / (int64_t)(esz * (size_t)ld)));
        DevBuf<void> tmp;
        HIPCHK(c, tmp.alloc(esz * (size_t)chunk_rows * (size_t)ld));
        int rc = DPMM_OK;
        for (int64_t r0 = 0; r0 < c->n && rc == DPMM_OK; r0 += chunk_rows) {
            const int64_t nr = std::min(chunk_rows, c->n - r0);
            hipError_t e = hipMemcpyAsync(tmp, (const char *)rows + esz * (size_t)r0 * (size_t)ld, esz * (size_t)nr * (size_t)ld, hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) e = launch_ingest_rows(c->dX + (size_t)r0 * c->ldx, c->ldx, tmp, is_f64, ld, nr, c->D, nan_to_zero, c->stream);
            if (e == hipSuccess) e = sync_stream(c, c->stream);       // tmp is reused by the next chunk
            if (e != hipSuccess) { c->err = std::string("dpmm_upload_points_npy: ") + hipGetErrorString(e); rc = DPMM_EHIP; }
        }
        if (rc != DPMM_OK) return rc;
        if (int rc2 = finish_upload(c)) return rc2;
    }
    c->have_points = true;
    c->cache_force = true;
    c->rows_full_K = -1;
    return DPMM_OK;
}

// the image the sparse sweep reads, into the buffer the dense Float32 kernel's fragment image lives in otherwise
static int pack_sparse_image(dpmm_ctx *c, const float *raw, float *Rp, int K) {
    HIPCHK(c, launch_mult_pack_sparse(raw, Rp, K, c->D, c->ldx, c->stream));
    return DPMM_OK;
}
static MultSparse sparse_args(const dpmm_ctx *c) {
    MultSparse sp{};
    sp.cp = c->d_cp; sp.ri = c->d_ri; sp.val = c->d_val; sp.T = c->d_Rp; sp.ticket = c->sb.ticket;
    return sp;
}

int dpmm_upload_points_csc(dpmm_ctx *c, const int64_t *colptr, const int64_t *rowval, const float *nzval, int index_base) {
    if (!c) return DPMM_EINVAL;
    if (c->prior != DPMM_PRIOR_MULT) return fail(c, DPMM_EINVAL, "dpmm_upload_points_csc: sparse points are for Multinomial contexts");
    if (c->D > DPMM_MAX_DIM_MULT_SPARSE) return fail(c, DPMM_ELIMIT, "dpmm_upload_points_csc: D > DPMM_MAX_DIM_MULT_SPARSE");
    if (index_base != 0 && index_base != 1) return fail(c, DPMM_EINVAL, "dpmm_upload_points_csc: index_base must be 0 or 1");
    if (!colptr) return fail(c, DPMM_EINVAL, "dpmm_upload_points_csc: colptr is null");
    const int64_t n = c->n;
    for (int64_t i = 0; i < n; ++i)
        if (colptr[i + 1] < colptr[i]) return fail(c, DPMM_EINVAL, "dpmm_upload_points_csc: colptr decreases at point " + std::to_string(i));
    const int64_t total = colptr[n] - colptr[0];
    if (total > 0 && (!rowval || !nzval)) return fail(c, DPMM_EINVAL, "dpmm_upload_points_csc: rowval / nzval is null");
    HIPCHK(c, hipSetDevice(c->device));
    // everything is built beside the points in force; they are replaced only when the new ones have passed the checks
    DevBuf<int64_t> t_cp, t_rv, n_cp;
    DevBuf<float> t_nz, n_val;
    DevBuf<uint16_t> n_ri;
    DevBuf<int32_t> t_cnt;
    DevBuf<unsigned long long> t_bad;
    std::vector<int32_t> cnt((size_t)n);
    std::vector<int64_t> ncp((size_t)n + 1, 0);
    unsigned long long bad = ~0ull;
    std::string msg;
    int rc = DPMM_OK;
    hipError_t e = n_cp.alloc(sizeof(int64_t) * ((size_t)n + 1));
    if (e == hipSuccess && n > 0) {
        const size_t tt = (size_t)std::max<int64_t>(total, 1);
        e = t_cp.alloc(sizeof(int64_t) * ((size_t)n + 1));
        if (e == hipSuccess) e = t_rv.alloc(sizeof(int64_t) * tt);
        if (e == hipSuccess) e = t_nz.alloc(sizeof(float) * tt);
        if (e == hipSuccess) e = t_cnt.alloc(sizeof(int32_t) * (size_t)n);
        if (e == hipSuccess) e = t_bad.alloc(sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMemcpyAsync(t_cp, colptr, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && total > 0) e = hipMemcpyAsync(t_rv, rowval, sizeof(int64_t) * (size_t)total, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && total > 0) e = hipMemcpyAsync(t_nz, nzval, sizeof(float) * (size_t)total, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(t_bad, 0xFF, sizeof(unsigned long long), c->stream);
        if (e == hipSuccess) e = launch_csc_check(t_cp, t_rv, t_nz, n, total, c->D, index_base, t_cnt, t_bad, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, t_bad, sizeof(bad), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(cnt.data(), t_cnt, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = sync_stream(c, c->stream);
        if (e == hipSuccess && bad != ~0ull) {
            rc = DPMM_EINVAL;
            msg = "dpmm_upload_points_csc: point " + std::to_string((long long)(bad >> 2)) +
                  ((bad & 3) == 1 ? ": row index out of range" : ": row indices are not strictly increasing (unsorted or duplicate)");
        }
        if (e == hipSuccess && rc == DPMM_OK) {
            for (int64_t i = 0; i < n; ++i) ncp[i + 1] = ncp[i] + cnt[i];      // explicit zeros are dropped
            const size_t nn = (size_t)std::max<int64_t>(ncp[n], 1);
            e = n_ri.alloc(sizeof(uint16_t) * nn);
            if (e == hipSuccess) e = n_val.alloc(sizeof(float) * nn);
            if (e == hipSuccess) e = hipMemcpyAsync(n_cp, ncp.data(), sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) e = launch_csc_compact(t_cp, t_rv, t_nz, n, index_base, n_cp, n_ri, n_val, c->stream);
            if (e == hipSuccess) e = sync_stream(c, c->stream);
        }
    } else if (e == hipSuccess) {
        e = hipMemsetAsync(n_cp, 0, sizeof(int64_t), c->stream);
        if (e == hipSuccess) e = sync_stream(c, c->stream);
    }
    if (e != hipSuccess || rc != DPMM_OK) {
        if (e != hipSuccess) return fail(c, DPMM_EHIP, std::string("dpmm_upload_points_csc: ") + hipGetErrorString(e));
        return fail(c, rc, msg);
    }
    t_cp.reset(); t_rv.reset(); t_nz.reset(); t_cnt.reset(); t_bad.reset();      // (before set_points_chunk sizes the slabs)
    c->dX.reset(); c->dX8.reset();
    c->d_cp = std::move(n_cp); c->d_ri = std::move(n_ri); c->d_val = std::move(n_val); c->nnz = ncp[n];
    c->x_sparse = 1; c->x_u8 = 0; c->x_bf16_exact = 0; c->repack_pending = false;
    if (int rc2 = set_points_chunk(c, true)) return rc2;
    if (c->have_params && c->d_raw) {       // parameters stay in force across an upload: the image the sparse sweep reads, from the raw rows
        if (int rc2 = pack_sparse_image(c, c->d_raw, c->d_Rp, c->K)) return rc2;
        c->rp_current = false;
        c->mspec_valid = false;
        HIPCHK(c, sync_stream(c, c->stream));
    }
    c->have_points = true;
    c->cache_force = true;
    c->rows_full_K = -1;
    return DPMM_OK;
}

int dpmm_init_labels(dpmm_ctx *c, int init_clusters, uint32_t epoch) {
    if (!c) return DPMM_EINVAL;
    if (init_clusters < 1 || init_clusters > DPMM_MAX_CLUSTERS) return fail(c, DPMM_ELIMIT, "init_clusters out of range");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n > 0) HIPCHK(c, launch_init_labels(c->dbins, c->n, c->first, init_clusters, 0, c->seed, epoch, c->stream));
    c->have_labels = true;
    c->rows_full_K = -1;
    return DPMM_OK;
}

int dpmm_init_labels_from(dpmm_ctx *c, int init_clusters, int first_label, uint32_t epoch) {
    if (!c) return DPMM_EINVAL;
    if (first_label < 1 || init_clusters < 1 || first_label - 1 + init_clusters > DPMM_MAX_CLUSTERS) return fail(c, DPMM_ELIMIT, "init_clusters / first_label out of range");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n > 0) HIPCHK(c, launch_init_labels(c->dbins, c->n, c->first, init_clusters, first_label - 1, c->seed, epoch, c->stream));
    c->have_labels = true;
    c->rows_full_K = -1;
    return DPMM_OK;
}

int dpmm_set_labels(dpmm_ctx *c, const int64_t *labels, const int64_t *sub) {
    if (!c) return DPMM_EINVAL;
    if (!c->have_labels && (!labels || !sub)) return fail(c, DPMM_ESTATE, "first dpmm_set_labels must provide both vectors");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0) { c->have_labels = true; return DPMM_OK; }
    DevBuf<int64_t> tmp;
    HIPCHK(c, tmp.alloc(sizeof(int64_t) * 2 * (size_t)c->n));
    int rc = DPMM_OK;
    hipError_t e = hipSuccess;
    if (labels) e = hipMemcpyAsync(tmp, labels, sizeof(int64_t) * c->n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && sub) e = hipMemcpyAsync(tmp + c->n, sub, sizeof(int64_t) * c->n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_bins_from_i64(c->dbins, labels ? tmp.get() : nullptr, sub ? tmp + c->n : nullptr, c->n, c->stream);
    if (e == hipSuccess) e = sync_stream(c, c->stream);
    if (e != hipSuccess) { c->err = std::string("dpmm_set_labels: ") + hipGetErrorString(e); rc = DPMM_EHIP; }
    else c->have_labels = true;
    c->rows_full_K = -1;
    return rc;
}

int dpmm_get_labels(dpmm_ctx *c, int64_t *labels, int64_t *sub) {
    if (!c) return DPMM_EINVAL;
    if (!c->have_labels) return fail(c, DPMM_ESTATE, "labels not initialised");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0) return DPMM_OK;
    DevBuf<int64_t> tmp;
    HIPCHK(c, tmp.alloc(sizeof(int64_t) * 2 * (size_t)c->n));
    hipError_t e = launch_bins_to_i64(c->dbins, tmp, tmp + c->n, c->n, c->stream);
    if (e == hipSuccess && labels) e = hipMemcpyAsync(labels, tmp, sizeof(int64_t) * c->n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && sub) e = hipMemcpyAsync(sub, tmp + c->n, sizeof(int64_t) * c->n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = sync_stream(c, c->stream);
    if (e != hipSuccess) { c->err = std::string("dpmm_get_labels: ") + hipGetErrorString(e); return DPMM_EHIP; }
    return DPMM_OK;
}

static int check_K(dpmm_ctx *c, int K) {
    if (K < 1) return fail(c, DPMM_EINVAL, "K < 1");
    if (K > DPMM_MAX_CLUSTERS) return fail(c, DPMM_ELIMIT, "K > DPMM_MAX_CLUSTERS");
    return DPMM_OK;
}

// ---- parameter staging: slot-indexed rows in pinned, GPU-addressable host memory ------------------------------------------
// Layout for `slots` clusters (Float32 unless noted):
//   NIW : mu [3 slots][D] | R [3 slots][D(D+1)/2] (packed upper triangle) | logdet [3 slots] | lr [slots][2] | w [slots] | cst [3 slots] | slot map Int32 [slots]
//   MULT:                   logp [3 slots][D]                   | lr [slots][2] | w [slots] | cst [3 slots] | slot map Int32 [slots]
struct ParLayout {
    size_t mu = 0, mat = 0, logdet = 0, lr = 0, w = 0, cst = 0, slot = 0, bytes = 0;
};
static ParLayout par_layout(const dpmm_ctx *c, int slots) {
    ParLayout L;
    const size_t D = (size_t)c->D, S = (size_t)slots;
    size_t o = 0;
    if (c->prior == DPMM_PRIOR_NIW) {
        // cst | mu | mat are contiguous (every offset a multiple of 16 bytes: slots is a multiple of 8): ONE copy takes them to the device
        L.cst = o; o += sizeof(float) * 3 * S;
        L.mu = o; o += sizeof(float) * 3 * S * D;
        L.mat = o; o += sizeof(float) * 3 * S * (D * (D + 1) / 2);
        L.logdet = o; o += sizeof(float) * 3 * S;
    } else {
        L.mat = o; o += sizeof(float) * 3 * S * D;
    }
    L.lr = o; o += sizeof(float) * 2 * S;
    L.w = o; o += sizeof(float) * S;
    if (c->prior != DPMM_PRIOR_NIW) { L.cst = o; o += sizeof(float) * 3 * S; }
    L.slot = o; o += sizeof(int32_t) * S;
    L.bytes = (o + 255) & ~(size_t)255;
    return L;
}

int dpmm_params_staging(dpmm_ctx *c, int slots, float **mu, float **mat, float **logdet, float **lr, float **w, int32_t **slot_of_cluster) {
    if (!c) return DPMM_EINVAL;
    if (slots < 1 || slots > DPMM_MAX_CLUSTERS) return fail(c, DPMM_ELIMIT, "slots out of range");
    HIPCHK(c, hipSetDevice(c->device));
    if (slots > c->par_slots) {
        int ns = std::max(8, c->par_slots);
        while (ns < slots) ns *= 2;
        ns = std::min(ns, DPMM_MAX_CLUSTERS);
        const ParLayout N = par_layout(c, ns);
        PinBuf<char> nb;
        HIPCHK(c, sync_stream(c, c->stream));      // a pack kernel may still read the old buffer
        if (int rc = regrow(c, nb, N.bytes, "dpmm_params_staging", "parameter staging")) return rc;
        memset(nb, 0, N.bytes);
        if (c->h_par) {                                  // contents are preserved (rows are slot-indexed: same offsets inside a region)
            const ParLayout O = par_layout(c, c->par_slots);
            const size_t D = (size_t)c->D, S = (size_t)c->par_slots;
            if (c->prior == DPMM_PRIOR_NIW) {
                memcpy(nb + N.mu, c->h_par + O.mu, sizeof(float) * 3 * S * D);
                memcpy(nb + N.mat, c->h_par + O.mat, sizeof(float) * 3 * S * (D * (D + 1) / 2));
                memcpy(nb + N.logdet, c->h_par + O.logdet, sizeof(float) * 3 * S);
            } else {
                memcpy(nb + N.mat, c->h_par + O.mat, sizeof(float) * 3 * S * D);
            }
            memcpy(nb + N.lr, c->h_par + O.lr, sizeof(float) * 2 * S);
            memcpy(nb + N.w, c->h_par + O.w, sizeof(float) * S);
            memcpy(nb + N.slot, c->h_par + O.slot, sizeof(int32_t) * S);
        }
        c->h_par = std::move(nb); c->par_slots = ns;
    }
    const ParLayout L = par_layout(c, c->par_slots);
    if (mu) *mu = c->prior == DPMM_PRIOR_NIW ? reinterpret_cast<float *>(c->h_par + L.mu) : nullptr;
    if (mat) *mat = reinterpret_cast<float *>(c->h_par + L.mat);
    if (logdet) *logdet = c->prior == DPMM_PRIOR_NIW ? reinterpret_cast<float *>(c->h_par + L.logdet) : nullptr;
    if (lr) *lr = reinterpret_cast<float *>(c->h_par + L.lr);
    if (w) *w = reinterpret_cast<float *>(c->h_par + L.w);
    if (slot_of_cluster) *slot_of_cluster = reinterpret_cast<int32_t *>(c->h_par + L.slot);
    return DPMM_OK;
}

static int direction_tables(dpmm_ctx *c, int K, bool b3_done, bool pb_done = false);

int dpmm_commit_params(dpmm_ctx *c, int K) {
    if (!c) return DPMM_EINVAL;
    if (int rc = check_K(c, K)) return rc;
    if (!c->h_par || K > c->par_slots) return fail(c, DPMM_ESTATE, "dpmm_commit_params: call dpmm_params_staging(slots >= K) first");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_capacity(c, K)) return rc;
    const ParLayout L = par_layout(c, c->par_slots);
    const float *hmu = reinterpret_cast<const float *>(c->h_par + L.mu), *hmat = reinterpret_cast<const float *>(c->h_par + L.mat);   // (NIW: re-pointed to the device copy below)
    const float *hld = reinterpret_cast<const float *>(c->h_par + L.logdet), *hlr = reinterpret_cast<const float *>(c->h_par + L.lr);
    const float *hw = reinterpret_cast<const float *>(c->h_par + L.w);
    float *hcst = reinterpret_cast<float *>(c->h_par + L.cst);
    const int32_t *hslot = reinterpret_cast<const int32_t *>(c->h_par + L.slot);
    const bool niw = c->prior == DPMM_PRIOR_NIW;
    for (int k = 0; k < K; ++k) {
        const int sl = hslot[k];
        if (sl < 0 || sl >= c->par_slots) return fail(c, DPMM_EINVAL, "slot_of_cluster entry out of range");
        // cst[3k] = -logdet/2 + log w_k ; cst[3k+1+s] = -logdet/2 + log lr_w[k][s]   (Float32, as the workers of the reference add them)
        hcst[3 * k] = (niw ? -0.5f * hld[3 * sl] : 0.f) + logf(hw[k]);
        hcst[3 * k + 1] = (niw ? -0.5f * hld[3 * sl + 1] : 0.f) + logf(hlr[2 * k]);
        hcst[3 * k + 2] = (niw ? -0.5f * hld[3 * sl + 2] : 0.f) + logf(hlr[2 * k + 1]);
    }
    // the kernels below read the staging buffer in place (no copy-engine transfer); the host may touch it again once a
    // blocking call (dpmm_step_stats, dpmm_suffstats_*, dpmm_sync) has returned
    if (niw) {
        // cst | mu | R of the slots in use: ONE streaming copy over the host link (1 KiB requests), then the gather into the fragment
        // images reads HBM.  (Letting the pack kernel gather from the pinned buffer directly cost 0.9 ms at D = 256 -- 16-byte
        // requests over PCIe -- against 0.25 ms for the bulk copy.)
        int top = 0;
        for (int k = 0; k < K; ++k) top = std::max(top, hslot[k] + 1);
        const size_t D = (size_t)c->D, T = D * (D + 1) / 2;
        const size_t img_bytes = (L.mat - L.cst) + sizeof(float) * 3 * (size_t)top * T;
        if (int rc = grow(c, c->d_par, (L.logdet - L.cst) + 1024, "dpmm_commit_params", "device copy of the parameter staging")) return rc;
        HIPCHK(c, launch_copy_bytes16(c->d_par, hcst, img_bytes, c->stream));
        const float *dcst = reinterpret_cast<const float *>(c->d_par.get());
        hmu = reinterpret_cast<const float *>(c->d_par + (L.mu - L.cst));
        hmat = reinterpret_cast<const float *>(c->d_par + (L.mat - L.cst));
        c->have_tail = c->opt_tail && c->D >= 4 && c->D % 4 == 0 && K > 1;
        HIPCHK(c, launch_niw_pack(hmat, hmu, c->d_Rp, c->d_mup, c->D, c->NB, 3 * K, c->have_tail ? c->d_tail : nullptr, dcst, hslot, c->d_cst,
                                  c->d_work, c->stream));
        c->work_zeroed = true;
        c->have_screen_prep = false;
        if (c->D > 16 && c->D <= 64 && K > 2) {
            // the vectorised far mask (64 clusters per step) pays once there are many clusters, or when the VALU tail
            // screen is unavailable (D not a multiple of 4); DPMM_OPT_PRESCREEN forces it off / on
            const bool want = c->opt_prescreen >= 0 ? c->opt_prescreen != 0 : (!c->have_tail || K > 64);
            if (want) {
                HIPCHK(c, launch_niw_screen_prep(hmat, hmu, c->D, K, c->d_lam, c->d_mdist, hslot, c->stream));
                c->have_screen_prep = true;
            }
        }
        c->predictive = false;          // (before the tables: direction_tables decides the three-plane images from it -- the first parameter set behind a
                                        //  dpmm_set_predictive_* call used to get none and drew one sweep's sub-labels with the Float32 chain: ADVICE r5)
        if (int rc = direction_tables(c, K, false)) return rc;
    } else {
        HIPCHK(c, launch_copy_bytes(c->d_cst, hcst, sizeof(float) * 3 * K, c->stream));
        HIPCHK(c, launch_gather_rows(c->d_raw, c->ldx, hmat, c->D, hslot, 3 * K, c->D, c->stream));
        if (c->x_sparse) { if (int rc = pack_sparse_image(c, c->d_raw, c->d_Rp, K)) return rc; }
        else HIPCHK(c, launch_mult_pack(c->d_raw, c->d_Rp, 3 * K, c->ldx, c->stream));
        c->rp_current = !c->x_sparse;
        if (c->x_u8) HIPCHK(c, launch_mult_pack_u8(c->d_raw, c->d_Lp16, 3 * K, c->ldx, c->ld8, c->stream));
        else if (c->x_bf16_exact) HIPCHK(c, launch_mult_pack_bf16(c->d_raw, c->d_Lp16, 3 * K, c->ldx, c->stream));
    }
    c->K = K;
    c->have_params = true;
    c->predictive = false;
    c->draws_on_device = false;
    return DPMM_OK;
}

// Direction screen: the tables of a new parameter set (one small kernel right behind the pack kernels, on the ctx stream).  Built only while
// it pays -- automatic mode: the tiles of the previous sweep kept eight or more candidates behind the 4-row tests on average (the waves
// write their counts into pinned memory; that sweep has been waited for by whoever brings new parameters), with hysteresis: on from 8 per
// tile, off below 4.  While it is on, the sweeps run the screen in front of the 4-row pair tests; the first sweep, every 32nd and the one
// after a change of K keep the usual order and count.
// h_need in words (g = sweep_grid_max workgroups of 4 waves): [0, 8 g) two words per wave of the general kernel | [8 g, 12 g) one word per wave of the lean
// kernel: tiles settled (low half), of them by the norm certificate (high half) | [12 g, 20 g) two words per wave of the lean kernel WITH the direction screen
static uint32_t *need_lean_settled(const dpmm_ctx *c) { return c->h_need + 8 * (size_t)c->sweep_grid_max; }
static uint32_t *need_lean_dir(const dpmm_ctx *c) { return c->h_need + 12 * (size_t)c->sweep_grid_max; }
static bool want_pair_ball(const dpmm_ctx *c, int K) { return c->opt_pair_ball && c->opt_ball && K >= 2 && K <= PB_MAXK; }      // (with the images: want_b3_images)
static bool want_b3_images(const dpmm_ctx *c) { return c->prior == DPMM_PRIOR_NIW && c->NB == 4 && c->opt_b3 && c->have_tail && !c->predictive; }
// The tight sn2 block of the pair-ball table costs the launch that writes it 19 us (hand-over 17.2 -> 36.1 us, K = 32 as K = 256: one workgroup per
// cluster); a tile settled by the norm certificate saves the lean launch 0.58 ns of its time (60 us for 103 000 tiles at N = 1e7).  DPMM_OPT_LEAN_NORM_CERT
// = 1 writes it only where that can come back: lean launch on, not the direction screen's regime (its instantiation runs no pair-ball test), at least
// 2^22 points, and -- once a sweep has reported -- at least 2^15 tiles settled by the certificate in the last sweep that had the block; else off for 63
// parameter sets.  Re-derived with sn2 for the neighbours: the block's cost is unchanged (the scalar squarings: 19 us), so the break-even stays
// 19 us / 0.58 ns = 32 800 = 2^15 settled tiles; the headline now settles 81 % (measured 0.56 ns per settled tile: lean launches 0.9316 -> 0.8606 ms for
// 126 600 tiles), which puts the break-even at 64 * 32 800 / 0.81 = 2.6e6 points (3.2e6 at 66 %): 2^21 is below it, 2^22 the first power of two above.  At
// the shard size (n = 1.25e6: 66 % of 19 500 tiles with the block, 23 % without) the step is 0.3089 ms with it against 0.2984 without: it stays without.  Without the block sn2 = sn and the certificate still runs, with the looser bound, for nothing.
// Called once per parameter set, before the launch that writes the table.  (Whatever it answers, labels and sub-labels are the same.)
static bool norm_tight(dpmm_ctx *c) {
    if (c->opt_lean_norm_cert >= 2) return true;
    if (!c->opt_lean_norm_cert) return false;
    if (c->cert_fb && c->sn2_tight) {
        unsigned long long cheap = 0;
        for (int w = 0; w < 4 * c->sweep_grid; ++w) cheap += need_lean_settled(c)[w] >> 16;
        if (cheap < (1ull << 15)) c->cert_cool = 64;
    }
    c->cert_fb = false;
    if (c->cert_cool > 0) { c->cert_cool -= 1; return false; }
    return c->opt_lean != 0 && c->lean_off == 0 && !c->sp_regime && c->n >= (int64_t)1 << 22;
}
static int direction_tables(dpmm_ctx *c, int K, bool b3_done, bool pb_done) {
    c->sp_ready = false;
    c->have_refb_big = false;
    c->have_b3 = false;
    if (want_b3_images(c)) {
        // the sub-cluster factors' bf16 planes + offsets (niw_lean.hip) -- b3_done: the hand-over launch wrote them (niw_master_pack_roles_kernel)
        // ... and the lean kernel's pair-ball table (same life as the images; one more row of workgroups of the same launch -- or a role of the hand-over launch)
        const bool pb = want_pair_ball(c, K);
        if (pb && !pb_done) c->sn2_tight = norm_tight(c);
        const int what = (b3_done ? 0 : 1) | ((pb && !pb_done) ? 2 : 0) | ((pb && !pb_done && c->sn2_tight) ? 4 : 0);
        if (what) HIPCHK(c, launch_niw_b3_pack(c->d_Rp, c->d_mup, K, c->d_tail, what, c->stream));
        c->have_b3 = true;
        c->have_pb = pb;
    } else c->have_pb = false;
    if (c->prior == DPMM_PRIOR_NIW && (c->NB == 8 || c->NB == 16) && c->d_refb_big && c->opt_bracket && c->have_tail && K > 1) {
        HIPCHK(c, launch_niw_refb_big(c->d_Rp, c->NB, K, c->d_refb_big, c->stream));      // D = 128, 256: the reference bracket's images
        c->have_refb_big = true;
    }
    if (c->prior != DPMM_PRIOR_NIW || c->NB != 4 || !c->d_sp_frag || K < 3 || K > SP_MAXK || !c->have_tail || !c->opt_bf16scr || c->opt_margin <= 0.f) return DPMM_OK;
    bool want = c->opt_direction > 0;
    if (c->opt_direction < 0) {
        unsigned long long many = 0, tiles = 0;
        const int nw = 4 * c->sweep_grid;
        unsigned long long many_ub = 0, tiles_ub = 0;        // sweeps that ran the screen in front of the tail pairs: counted there, an upper bound
        unsigned long long given = 0, removed = 0;            // the last sweep's direction screens, if it ran any
        bool lean_dir = false;                                // ... in the lean kernel
        for (int w = 0; w < nw; ++w) {
            const uint32_t v = c->h_need[2 * w];
            if (v & 0x8000u) { many_ub += v >> 16; tiles_ub += v & 0x7FFFu; } else { many += v >> 16; tiles += v & 0x7FFFu; }
            if (c->sp_last) { const uint32_t y = c->h_need[2 * w + 1]; given += y & 0xFFFFu; removed += y >> 16; }
            tiles += need_lean_settled(c)[w] & 0xFFFFu;      // tiles niw_lean_kernel settled (no candidate behind the 4-row tests)
            // ... and the tiles it settled WITH the direction screen: their candidates and the screen's yield, in the general kernel's format
            const uint32_t v3 = need_lean_dir(c)[2 * w], y3 = need_lean_dir(c)[2 * w + 1];
            if (v3 & 0x8000u) { many_ub += v3 >> 16; tiles_ub += v3 & 0x7FFFu; } else { many += v3 >> 16; tiles += v3 & 0x7FFFu; }
            given += y3 & 0xFFFFu; removed += y3 >> 16;
            if (y3) lean_dir = true;
        }
        memset(c->h_need, 0, sizeof(uint32_t) * 2 * (size_t)nw);
        memset(need_lean_settled(c), 0, sizeof(uint32_t) * (size_t)nw);      // (read once: a later launch on a smaller grid, or one that does not count, leaves zeros -- "no tiles")
        memset(need_lean_dir(c), 0, sizeof(uint32_t) * 2 * (size_t)nw);
        // (break-even measured on the growth run: at 4.3 candidates per tile the screen costs 3 % of the step, at 28 it saves a third)
        if (tiles > 0) c->sp_regime = c->sp_regime ? (many >= tiles * 4) : (many >= tiles * 8);
        else if (tiles_ub > 0 && many_ub < tiles_ub * 4) c->sp_regime = false;        // even the upper bound is below the switch-off level
        // clusters that overlap along every direction (a chain that is still growing: one cluster over several components): the screen is
        // given candidates and removes few -- off for 64 parameter sets, then it may try again
        if ((c->sp_last || lean_dir) && given > 0 && removed * 4 < given) { c->sp_regime = false; c->sp_cooldown = 64; }
        if (c->sp_cooldown > 0) { c->sp_cooldown -= 1; c->sp_regime = false; }
        want = c->sp_regime;
    }
    c->sp_last = false;
    if (!want) { c->sp_count = 0; return DPMM_OK; }
    c->sp_count = (K != c->sp_K) ? 1u : c->sp_count + 1u;      // (a new number of clusters: measure again)
    c->sp_K = K;
    HIPCHK(c, launch_niw_direction(c->d_Rp, c->d_mup, c->d_cst, c->D, K, c->d_sp_frag, c->d_sp_cons, c->stream));
    c->sp_ready = true;
    return DPMM_OK;
}

// compat entry points: copy the caller's cluster-ordered arrays into the staging rows (identity slot map) and commit
static int stage_and_commit(dpmm_ctx *c, int K, const float *mu, const float *mat, const float *logdet, const float *lr, const float *w) {
    float *smu, *smat, *sld, *slr, *sw;
    int32_t *sslot;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_stream(c, c->stream));          // an earlier pack kernel may still read the staging buffer
    if (int rc = dpmm_params_staging(c, K, &smu, &smat, &sld, &slr, &sw, &sslot)) return rc;
    const size_t D = (size_t)c->D;
    if (mu) memcpy(smu, mu, sizeof(float) * 3 * K * D);
    if (c->prior == DPMM_PRIOR_NIW) {       // full row-major R from the caller -> the packed upper triangle of the staging rows
        const size_t T = D * (D + 1) / 2;
        for (size_t j = 0; j < 3 * (size_t)K; ++j)
            for (size_t r = 0; r < D; ++r) memcpy(smat + j * T + r * D - r * (r - 1) / 2, mat + (j * D + r) * D + r, sizeof(float) * (D - r));
    } else {
        memcpy(smat, mat, sizeof(float) * 3 * K * D);
    }
    if (logdet) memcpy(sld, logdet, sizeof(float) * 3 * K);
    memcpy(slr, lr, sizeof(float) * 2 * K);
    memcpy(sw, w, sizeof(float) * K);
    for (int k = 0; k < K; ++k) sslot[k] = k;
    return dpmm_commit_params(c, K);
}

int dpmm_set_params_niw_chol(dpmm_ctx *c, int K, const float *mu, const float *R, const float *logdet, const float *lr, const float *w) {
    if (!c) return DPMM_EINVAL;
    if (c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, "context was created for another prior");
    if (!mu || !R || !logdet || !lr || !w) return fail(c, DPMM_EINVAL, "null parameter array");
    if (int rc = check_K(c, K)) return rc;
    return stage_and_commit(c, K, mu, R, logdet, lr, w);
}

int dpmm_set_params_niw(dpmm_ctx *c, int K, const float *mu, const float *inv_sigma, const float *logdet, const float *lr, const float *w) {
    if (!c) return DPMM_EINVAL;
    if (c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, "context was created for another prior");
    if (!inv_sigma) return fail(c, DPMM_EINVAL, "null parameter array");
    if (int rc = check_K(c, K)) return rc;
    // compat path: Sigma^-1 = R'R (upper Cholesky factor) in Float64 on the host
    const int D = c->D;
    std::vector<float> R((size_t)3 * K * D * D, 0.f);
    std::vector<double> L((size_t)D * D);
    for (int j = 0; j < 3 * K; ++j) {
        const float *A = inv_sigma + (size_t)j * D * D;
        std::fill(L.begin(), L.end(), 0.0);
        for (int a = 0; a < D; ++a) {  // lower factor, row by row
            for (int b = 0; b <= a; ++b) {
                double s = 0.5 * ((double)A[(size_t)a * D + b] + (double)A[(size_t)b * D + a]);
                for (int t = 0; t < b; ++t) s -= L[(size_t)a * D + t] * L[(size_t)b * D + t];
                L[(size_t)a * D + b] = (a == b) ? std::sqrt(s) : s / L[(size_t)b * D + b];
            }
        }
        float *Rj = R.data() + (size_t)j * D * D;
        for (int a = 0; a < D; ++a)
            for (int b = a; b < D; ++b) Rj[(size_t)a * D + b] = (float)L[(size_t)b * D + a];  // R = L'
    }
    return dpmm_set_params_niw_chol(c, K, mu, R.data(), logdet, lr, w);
}

int dpmm_set_params_mult(dpmm_ctx *c, int K, const float *logp, const float *lr, const float *w) {
    if (!c) return DPMM_EINVAL;
    if (c->prior != DPMM_PRIOR_MULT) return fail(c, DPMM_EINVAL, "context was created for another prior");
    if (!logp || !lr || !w) return fail(c, DPMM_EINVAL, "null parameter array");
    if (int rc = check_K(c, K)) return rc;
    return stage_and_commit(c, K, nullptr, logp, nullptr, lr, w);
}

int dpmm_set_num_clusters(dpmm_ctx *c, int K) {
    if (!c) return DPMM_EINVAL;
    if (int rc = check_K(c, K)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_capacity(c, K)) return rc;
    if (K != c->K) c->have_params = false;
    c->K = K;
    return DPMM_OK;
}

int dpmm_num_clusters(const dpmm_ctx *c) { return c ? c->K : 0; }

int dpmm_numa_node(dpmm_ctx *c) {
    if (!c) return -1;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), c->device) != hipSuccess) return -1;
    for (char *p = bus; *p; ++p) if (*p >= 'A' && *p <= 'F') *p = (char)(*p - 'A' + 'a');      // sysfs uses lower-case hex
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
    FILE *f = fopen(path.c_str(), "r");
    if (!f) return -1;
    int node = -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    return node;
}

static int noise_flush(dpmm_ctx *c);

// ---- run_sweep's NIW branch in three parts.  (1) The argument block every launch of the sweep shares -- and, at D = 128, 256, the bracket launch in
// front of the sweep, whose output the block then names.
static int niw_sweep_args(dpmm_ctx *c, NiwSweepArgs &a, uint32_t epoch, int final_argmax, float *table, int64_t table_stride, bool ranged, int64_t p0, int64_t rn, int64_t rtiles) {
    a.X = (ranged && c->dX) ? c->dX + p0 * c->ldx : c->dX; a.ldx = c->ldx; a.n = rn; a.first_index = c->first + p0; a.ntiles = rtiles; a.K = c->K;
    a.Rp = c->d_Rp; a.mup = c->d_mup; a.cst = c->d_cst;
    a.tdf = c->predictive ? c->d_tdf : nullptr;
    a.scratch = table ? table : c->d_scratch; a.scratch_stride = table ? table_stride : c->scratch_stride;
    a.scratch_by_tile = table ? 1 : 0; a.labels_only = table ? 1 : 0;
    a.bins = c->dbins; a.seed = c->seed; a.epoch = epoch; a.final_argmax = final_argmax;
    a.screen_margin = table ? 0.f : c->opt_margin;
    a.use_prev = (c->have_labels && !ranged) ? 1 : 0;      // (a range: bins stays unshifted and must not be read, not even as a prefetch hint)
    a.lam = (c->have_screen_prep && !c->predictive) ? c->d_lam : nullptr;
    a.mdist = c->d_mdist;
    a.tail = (c->have_tail && !c->predictive) ? c->d_tail : nullptr;
    a.tail_g = ((c->D - 4) % 16) / 4;
    a.ball = c->opt_ball ? NIW_BALL_ON : 0; a.bracket = c->opt_bracket;
    a.bf16scr = (c->opt_bf16scr && c->NB == 4 && a.tail != nullptr) ? NIW_SCR_ON : 0;
    if (c->sp_ready && a.bf16scr && !table && !final_argmax) {
        a.sp_frag = c->d_sp_frag; a.sp_cons = c->d_sp_cons;
        // the DIR kernel -- the one that writes the yield words -- runs (store_labels only waives Student-t mode, which never meets the bf16 screens)
        c->sp_last = niw_steady_launch(a, false) && niw_dir_screen(a);
        if (c->opt_direction > 0 || c->sp_count % 32u != 1u) a.bf16scr |= NIW_SCR_DIR_FIRST;
    }
    a.need = (table || c->opt_direction == 0) ? nullptr : c->h_need;
    // the visiting order is set BEFORE the bracket launch: its tiles and thresholds are indexed by visiting position and
    // must be those the sweep walks (a bracket computed in storage order would hand a point another point's threshold)
    a.order = (!table && c->have_perm && c->opt_ordered) ? c->sb.perm : nullptr; a.order_total = c->sb.perm_total;
    if (c->have_refb_big && a.tail != nullptr && !table && a.bracket && a.use_prev && a.screen_margin > 0.f && !final_argmax) {
        // D = 128, 256: the reference bracket as a launch of its own in front of the sweep (niw_bracket_big_kernel): per tile whether all
        // its points were in one cluster, per point the lower end of a certified bracket of that cluster's value
        if (!c->d_brk_flag) {
            const size_t nt = (size_t)((c->n + 127) / 128);
            HIPCHK(c, c->d_brk_flag.alloc(sizeof(uint32_t) * std::max<size_t>(nt, 1)));
            HIPCHK(c, c->d_brk_aref.alloc(sizeof(float) * std::max<size_t>(nt * 128, 1)));
        }
        HIPCHK(c, launch_niw_bracket_big(c->NB, a, c->d_refb_big, c->d_brk_flag, c->d_brk_aref, c->stream));
        a.brk_flag = c->d_brk_flag; a.brk_aref = c->d_brk_aref;
    }
    a.work = table ? nullptr : c->d_work;
    if (!table) { c->work_waves = std::max(c->work_waves, 4 * c->sweep_grid); c->work_launches += 1; }
    a.prio = c->opt_prio; a.queue_rounds = c->opt_queue_rounds;
#ifdef DPMM_STAMPS
    if (!g_dbg) { hipMalloc(&g_dbg, sizeof(unsigned long long) * 16 * 4 * 4096); hipMemset(g_dbg, 0, sizeof(unsigned long long) * 16 * 4 * 4096); }
    a.dbg = g_dbg;
#endif
    return DPMM_OK;
}

// (2) Does this label-storing sweep start with the lean kernel?  niw_lean_kernel settles the tiles the cheap screens settle completely, labels and
// sub-labels in one go, and leaves the others on a list.  A sweep that left more than 30 % of its tiles (overlapping clusters: the screens' later stages
// do the work) switches it off for lean_backoff sweeps -- every path gives the same labels and sub-labels, so the decision is free to be local.  The
// verdict is on the last sweep that ran it: h_hard[0], the length of the list it left.  (The lean kernel runs the direction screen itself while the
// tables exist, unless DPMM_OPT_LEAN_DIRECTION is off: then it stays out of that regime.)
static bool lean_this_sweep(dpmm_ctx *c, const NiwSweepArgs &a) {
    const bool lean_ok = c->opt_lean != 0 && c->opt_bracket && a.use_prev && a.screen_margin > 0.f && !a.final_argmax && a.lam == nullptr && c->K > 1 && c->d_hard &&
                         !(c->opt_lean_dir == 0 && c->sp_regime && c->opt_direction != 0 && c->sp_ready);
    if (!lean_ok) return false;
    if (c->lean_off == 0 && c->lean_ran) {
        const int64_t nwt = (c->n + 63) / 64;
        if ((int64_t)c->h_hard[0] * 10 > nwt * 3) { c->lean_off = c->lean_backoff; c->lean_backoff = std::min(2 * c->lean_backoff + 1, 1023); }
        else c->lean_backoff = 15;
        c->lean_ran = false;
    }
    if (c->lean_off > 0) { c->lean_off -= 1; c->h_hard[0] = 0; return false; }
    c->lean_ran = true;
    return true;
}

// (3) The sweep's launches while the bf16 sub-label evaluation is active (niw_lean.hip), with their part events: lean kernel (if asked for) -> the sweep
// kernel on the list it left, or on every tile: it draws and STORES the labels (LSTORE instantiations) -> the sub-labels of every tile where no list was
// walked (a list's spans were finished by the LIST launch) -- every sub-cluster value of a sweep then comes from the same arithmetic.
static int niw_label_store_chain(dpmm_ctx *c, const NiwSweepArgs &a, bool use_lean) {
    const bool parts = (c->opt_timing & 8) != 0 && (c->opt_timing & 1) != 0;
    if (parts && !c->ev_part[0]) for (auto &e : c->ev_part) HIPCHK(c, hipEventCreate(&e));
    NiwLabelStore ls{true};
    if (use_lean) {
        const size_t hw = hard_list_words(c->n);
        uint32_t *mine = c->d_hard + (size_t)c->hard_flip * hw, *other = c->d_hard + (size_t)(c->hard_flip ^ 1) * hw;
        c->hard_flip ^= 1;
        uint32_t *need2 = a.need ? need_lean_settled(c) : nullptr, *need3 = a.need ? need_lean_dir(c) : nullptr;
        // (tiles aligned to the bins of the sort that wrote the visiting order, when there is one and it fits the kernel's table)
        const bool al = a.order != nullptr && c->perm_nbins > 0 && c->perm_nbins <= NIW_LEAN_MAX_BINS;
        NiwSweepArgs al_args = a;
        if (!c->opt_lean_dir) { al_args.sp_frag = nullptr; al_args.sp_cons = nullptr; }
        if (c->have_pb && c->opt_pair_ball && al_args.ball) {
            al_args.ball |= NIW_BALL_PAIR_TABLE;
            if (c->opt_lean_norm_cert) al_args.ball |= NIW_BALL_NORM_CERT;
            if (c->opt_lean_norm_cert == 3) al_args.ball |= NIW_BALL_NB_LOOSE;
        }
        c->cert_fb = need2 != nullptr && (al_args.ball & NIW_BALL_NORM_CERT) != 0 && !(al_args.sp_frag && al_args.sp_cons);
#ifndef DPMM_STAMPS
        al_args.cert_points = c->d_cert_rec;
#endif
        HIPCHK(c, launch_niw_lean(al_args, mine, need2, other, al ? c->sb.bin_start : nullptr, al ? c->perm_nbins : 0, need3, c->sweep_grid, c->stream));
        if (parts) HIPCHK(c, hipEventRecord(c->ev_part[0], c->stream));
        ls.tile_list = mine;
        ls.list_len = c->h_hard;
    }
    HIPCHK(c, launch_niw_sweep(c->NB, a, c->sweep_grid, c->stream, ls));
    if (parts) HIPCHK(c, hipEventRecord(c->ev_part[1], c->stream));
    c->have_parts = parts ? (use_lean ? 2 : 1) : 0;
    if (!ls.tile_list) HIPCHK(c, launch_niw_sub(a, nullptr, nullptr, c->sweep_grid, c->stream));
    return DPMM_OK;
}

// Table mode takes a range of the points, [p0, p0 + np) with p0 a multiple of the tile (np < 0: all of them, the launch every caller but the
// scoring entry points makes): the kernels see shifted base pointers, n = np and the range's tiles, and write table column 0 for point p0.
// Table mode draws nothing and visits in storage order; the sparse columns' offsets are absolute, so shifting cp is enough.  What stays
// unshifted is not per point or not read: mdist, tail and the parameter images are per cluster; bins (the previous labels: a prefetch /
// row-block hint outside table mode) is switched off for a range with use_prev = 0; the table kernels write no label.
static int run_sweep(dpmm_ctx *c, uint32_t epoch, int final_argmax, float *table, int64_t table_stride, int64_t p0 = 0, int64_t np = -1) {
    if (!c->have_points || !c->have_params) return fail(c, DPMM_ESTATE, "sweep needs points and parameters");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0) return DPMM_OK;
    const bool ranged = np >= 0;
    if (ranged && (!table || p0 < 0 || p0 % c->tile != 0 || np == 0 || p0 + np > c->n)) return fail(c, DPMM_EINVAL, "run_sweep: bad point range");
    const int64_t rn = ranged ? np : c->n;
    const int64_t rtiles = ranged ? (np + c->tile - 1) / c->tile : c->ntiles;
    const int rgrid = ranged ? (int)std::min<int64_t>(c->sweep_grid, rtiles) : c->sweep_grid;
    if (c->prior == DPMM_PRIOR_NIW && !table) {
        if (!c->work_zeroed) HIPCHK(c, hipMemsetAsync(c->d_work, 0, sizeof(unsigned long long) * DPMM_WORK_SLOTS, c->stream));   // usually done by the pack kernel
        c->work_zeroed = false;
    }
    if (!table && (c->opt_timing & 1)) HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    if (c->prior == DPMM_PRIOR_NIW) {
        NiwSweepArgs a{};
        if (int rc = niw_sweep_args(c, a, epoch, final_argmax, table, table_stride, ranged, p0, rn, rtiles)) return rc;
        const bool b3 = c->NB == 4 && c->have_b3 && c->opt_b3 && !table && !c->predictive && a.tail != nullptr;
        if (b3) {
            if (int rc = niw_label_store_chain(c, a, lean_this_sweep(c, a))) return rc;
        } else {
            HIPCHK(c, launch_niw_sweep(c->NB, a, rgrid, c->stream));
            if (!table) c->have_parts = 0;          // (a one-launch sweep records no part events: dpmm_last_sweep_parts_ms must not mix its ev[0] / ev[1] with an older sweep's)
        }
    } else {
        MultSweepArgs a{};
        a.X = (ranged && c->dX) ? c->dX + p0 * c->ldx : c->dX; a.ldx = c->ldx; a.n = rn; a.first_index = c->first + p0; a.D = c->D; a.K = c->K;
        a.logp = c->d_Rp; a.cst = c->d_cst;
        a.scratch = table ? table : c->d_scratch;
        a.scratch_stride = table ? table_stride : c->scratch_stride;
        a.scratch_by_tile = table ? 1 : 0;
        a.labels_only = table ? 1 : 0;
        a.bins = c->dbins; a.seed = c->seed; a.epoch = epoch; a.final_argmax = final_argmax;
        a.use_prev = (c->have_labels && !ranged) ? 1 : 0;
        a.order = (!table && c->have_perm && c->opt_ordered) ? c->sb.perm : nullptr;
        a.order_total = c->sb.perm_total;
        if (c->x_sparse) { MultSparse sp = sparse_args(c); sp.cp += p0; HIPCHK(c, launch_mult_sweep_sparse(a, sp, rgrid, c->stream)); }
        else if (c->x_u8) HIPCHK(c, launch_mult_sweep_u8(a, c->dX8 + p0 * c->ld8, c->ld8, c->d_Lp16, rgrid, c->stream));
        else if (c->x_bf16_exact) HIPCHK(c, launch_mult_sweep_bf16(a, c->d_Lp16, rgrid, c->stream));
        else {
            if (!c->rp_current) { HIPCHK(c, launch_mult_pack(c->d_raw, c->d_Rp, 3 * c->K, c->ldx, c->stream)); c->rp_current = true; }      // (skipped by a device-master draw)
            HIPCHK(c, launch_mult_sweep(a, rgrid, c->stream));
        }
    }
    if (!table) {
        if (c->master) if (int rc = noise_flush(c)) return rc;
        if (c->opt_timing & 1) HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
        c->have_sweep_ev = (c->opt_timing & 1) != 0;
        c->have_labels = true;
    }
    return DPMM_OK;
}

int dpmm_sweep(dpmm_ctx *c, uint32_t epoch, int final_argmax) {
    if (!c) return DPMM_EINVAL;
    if (c->predictive) return fail(c, DPMM_ESTATE, "predictive parameters are loaded: set the sweep parameters again");
    return run_sweep(c, epoch, final_argmax, nullptr, 0);
}

int dpmm_set_predictive_niw(dpmm_ctx *c, int K, const float *m, const float *R, const float *logdet, const float *df, const float *w) {
    if (!c) return DPMM_EINVAL;
    if (c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, "context was created for another prior");
    if (!m || !R || !logdet || !df || !w) return fail(c, DPMM_EINVAL, "null parameter array");
    if (int rc = check_K(c, K)) return rc;
    const size_t D = (size_t)c->D;
    // expand to the (cluster, left, right) row layout of the sweep kernels; only rows 3k are read in table mode
    std::vector<float> mu3(3 * K * D, 0.f), R3(3 * K * D * D, 0.f), ld3(3 * (size_t)K, 0.f), lr(2 * (size_t)K, 0.5f);
    for (int k = 0; k < K; ++k) {
        memcpy(&mu3[(size_t)3 * k * D], m + (size_t)k * D, sizeof(float) * D);
        memcpy(&R3[(size_t)3 * k * D * D], R + (size_t)k * D * D, sizeof(float) * D * D);
    }
    if (int rc = dpmm_set_params_niw_chol(c, K, mu3.data(), R3.data(), ld3.data(), lr.data(), w)) return rc;
    // MvTDist log-density constant: lgamma((df+D)/2) - lgamma(df/2) - D/2 log(df pi) - logdet(Sigma)/2 + log w
    std::vector<float> cst(3 * (size_t)K, 0.f), tdf(6 * (size_t)K, 1.f);
    for (int k = 0; k < K; ++k) {
        const double v = df[k];
        cst[3 * k] = (float)(lgamma(0.5 * (v + D)) - lgamma(0.5 * v) - 0.5 * D * log(v * M_PI) - 0.5 * logdet[k] + log((double)w[k]));
        tdf[6 * k] = (float)v;
        tdf[6 * k + 1] = (float)(0.5 * (v + D));
    }
    if (int rc = ensure_pinned(c, sizeof(float) * 9 * K)) return rc;
    HIPCHK(c, sync_stream(c, c->stream));
    memcpy(c->h_pin, cst.data(), sizeof(float) * 3 * K);
    memcpy(c->h_pin + sizeof(float) * 3 * K, tdf.data(), sizeof(float) * 6 * K);
    HIPCHK(c, launch_copy_bytes(c->d_cst, c->h_pin, sizeof(float) * 3 * K, c->stream));
    HIPCHK(c, launch_copy_bytes(c->d_tdf, c->h_pin + sizeof(float) * 3 * K, sizeof(float) * 6 * K, c->stream));
    HIPCHK(c, sync_stream(c, c->stream));
    c->predictive = true;
    // include/dpmm_hip_missing.h: the constant of the marginal over D - r features, r = 1 .. DPMM_SCORE_MAX_MISSING (host memory only: the device
    // copies are made by the first call that marginalises)
    c->h_miss_cst.assign((size_t)K * MISS_CST, 0.0);
    for (int k = 0; k < K; ++k) {
        const double v = df[k];
        double *ck = &c->h_miss_cst[(size_t)k * MISS_CST];
        ck[0] = v;
        for (int r = 1; r <= MISS_MAX && r < (int)D; ++r) {
            const double Do = (double)((int)D - r);
            ck[r] = lgamma(0.5 * (v + Do)) - lgamma(0.5 * v) - 0.5 * Do * log(v * M_PI) - 0.5 * logdet[k] + log((double)w[k]);
        }
    }
    c->miss_slots = c->par_slots;
    c->pred_gen += 1;
    return DPMM_OK;
}

int dpmm_set_predictive_mult(dpmm_ctx *c, int K, const float *logp, const float *w) {
    if (!c) return DPMM_EINVAL;
    if (c->prior != DPMM_PRIOR_MULT) return fail(c, DPMM_EINVAL, "context was created for another prior");
    if (!logp || !w) return fail(c, DPMM_EINVAL, "null parameter array");
    if (int rc = check_K(c, K)) return rc;
    const size_t D = (size_t)c->D;
    std::vector<float> lp3(3 * K * D, 0.f), lr(2 * (size_t)K, 0.5f);
    for (int k = 0; k < K; ++k) memcpy(&lp3[(size_t)3 * k * D], logp + (size_t)k * D, sizeof(float) * D);
    if (int rc = dpmm_set_params_mult(c, K, lp3.data(), lr.data(), w)) return rc;
    c->predictive = true;
    c->pred_gen += 1;
    return DPMM_OK;
}

int dpmm_predict(dpmm_ctx *c, float *parr) {
    if (!c || !parr) return DPMM_EINVAL;
    if (!c->predictive) return fail(c, DPMM_ESTATE, "dpmm_predict needs dpmm_set_predictive_* first");
    return dpmm_debug_loglik(c, parr);
}

int dpmm_predict_points(dpmm_ctx *c, int64_t *labels, float *probs) {
    if (!c || !labels) return DPMM_EINVAL;
    if (!c->predictive) return fail(c, DPMM_ESTATE, "dpmm_predict_points needs dpmm_set_predictive_* first");
    if (!c->have_points || !c->have_params) return fail(c, DPMM_ESTATE, "predict needs points and parameters");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0) return DPMM_OK;
    const int64_t stride = c->ntiles * c->tile;
    const int rstep = (c->prior == DPMM_PRIOR_NIW) ? 1 : 3;       // Multinomial: rows 3k are the cluster-level rows
    DevBuf<float> table, d_probs;
    DevBuf<int64_t> d_lab;
    HIPCHK(c, table.alloc(sizeof(float) * (size_t)(rstep * c->K) * (size_t)stride));
    int rc = run_sweep(c, 0, 0, table, stride);
    hipError_t e = hipSuccess;
    if (rc == DPMM_OK) {
        e = d_lab.alloc(sizeof(int64_t) * (size_t)c->n);
        if (e == hipSuccess && probs) e = d_probs.alloc(sizeof(float) * (size_t)c->n * (size_t)c->K);
        if (e == hipSuccess) e = launch_predict_finish(table, stride, rstep, c->n, c->K, d_lab, d_probs, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(labels, d_lab, sizeof(int64_t) * (size_t)c->n, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && probs) e = hipMemcpyAsync(probs, d_probs, sizeof(float) * (size_t)c->n * (size_t)c->K, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = sync_stream(c, c->stream);
        if (e != hipSuccess) { c->err = std::string("dpmm_predict_points: ") + hipGetErrorString(e); rc = DPMM_EHIP; }
    }
    return rc;
}

int dpmm_debug_loglik(dpmm_ctx *c, float *out) {
    if (!c || !out) return DPMM_EINVAL;
    if (!c->have_points || !c->have_params) return fail(c, DPMM_ESTATE, "debug_loglik needs points and parameters");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0) return DPMM_OK;
    const int64_t stride = c->ntiles * c->tile;
    const int rows = (c->prior == DPMM_PRIOR_NIW) ? c->K : 3 * c->K;
    DevBuf<float> table;
    HIPCHK(c, table.alloc(sizeof(float) * (size_t)rows * (size_t)stride));
    int rc = run_sweep(c, 0, 0, table, stride);
    if (rc == DPMM_OK) {
        // Multinomial: rows 3k of the 3K-row table are the cluster-level rows
        const size_t src_pitch = sizeof(float) * stride * (c->prior == DPMM_PRIOR_MULT ? 3 : 1);
        hipError_t e = hipMemcpy2DAsync(out, sizeof(float) * c->n, table, src_pitch, sizeof(float) * c->n,
                                        (size_t)c->K, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = sync_stream(c, c->stream);
        if (e != hipSuccess) { c->err = std::string("dpmm_debug_loglik: ") + hipGetErrorString(e); rc = DPMM_EHIP; }
        else if (c->opt_ref_const && c->prior == DPMM_PRIOR_NIW && !c->predictive) {
            // mv_gaussian.jl:24 normalises with length(Sigma) = D^2: -(D^2 log 2 pi + logdet)/2; the table carries -logdet/2 only
            const float k2pi = (float)(-0.5 * (double)c->D * (double)c->D * log(2.0 * M_PI));
            for (size_t i = 0; i < (size_t)c->K * (size_t)c->n; ++i) out[i] += k2pi;
        }
    }
    return rc;
}

int64_t dpmm_packed_stride(const dpmm_ctx *c) { return c ? c->packed_stride : 0; }

// statistics output (rows | flags) in pinned memory.  Growing it waits for the stream: rows announced as late have arrived by then
static inline int ensure_out(dpmm_ctx *c, size_t bytes) {
    if (bytes <= c->h_out.bytes) return DPMM_OK;
    HIPCHK(c, sync_stream(c, c->stream));
    c->rows_late = false;
    return regrow(c, c->h_out, bytes, "dpmm", "pinned statistics rows", (size_t)1 << 20);
}

// One-collective pass: the sub-labels of this shard's candidates that turned out not to be bad go back to the side they were on.  Labels
// only -- nothing the master waits for -- so the kernel is queued behind the posteriors / the copy of the rows, before the call returns
// (every later reader of the labels is stream-ordered behind it).
static int flush_undo(dpmm_ctx *c) {
    if (!c->undo_pending) return DPMM_OK;
    c->undo_pending = false;
    const uint8_t *flags = reinterpret_cast<const uint8_t *>(c->d_out.get()) + sizeof(double) * 2 * (size_t)c->K * (size_t)c->packed_stride;
    HIPCHK(c, launch_niw_undo_reset(c->dbins, c->n, c->K, flags, c->d_cside, c->stream));
    return DPMM_OK;
}
// One statistics pass on the ctx stream (asynchronous): [sub-cluster occupancies -> bad-cluster reset ->] sort by bin ->
// segmented statistics -> packed rows in c->d_out [-> all-reduce over the ranks].
// with_reset (the per-step pass) has two forms when a communicator is attached:
//   two collectives (DPMM_OPT_ONE_COLLECTIVE = 0, Multinomial): histogram -> ALL-REDUCE of the 2K Int64 occupancies -> flags + reset +
//       re-count -> scan / scatter -> statistics -> ALL-REDUCE of the 2K packed rows.  The first collective sits in the middle of the sort chain.
//   one collective (NIW, default): the reset is applied SPECULATIVELY to this shard's candidates -- clusters with exactly one empty
//       sub-cluster HERE; a cluster that is bad globally is a candidate on every rank that holds points of it -- and ONE ALL-REDUCE
//       carries 3K rows: the 2K rows of the labels AS SWEPT (for a candidate: everything on the side its points were on, rebuilt from
//       left' + right') and K re-drawn left rows X.  Behind it niw_finalize_rows_kernel reads the verdict off the rows' own N column:
//       bad cluster -> (X, left + right - X), anything else -> the rows as they are; a shard's candidate that is not bad gets its
//       sub-labels back (all of its points were on one side).  No history, no second pass, 1.5x the bytes of a 1.1 MB message.
//   Same end state as the reference's full pass + subset pass (update_suff_stats_posterior! + reset_bad_clusters!,
//   src/local_clusters_actions.jl:665-666, 501-516) either way; tests/test_gpu_multirank.py: the chains are the one-rank chain.
static int run_stats(dpmm_ctx *c, const int64_t *idx, int n_idx, bool with_reset = false, uint32_t reset_epoch = 0, uint8_t *flags_to = nullptr,
                     bool *flags_sent = nullptr) {
    if (!c->have_points || !c->have_labels || c->K < 1) return fail(c, DPMM_ESTATE, "suffstats need points, labels and parameters (K)");
    HIPCHK(c, hipSetDevice(c->device));
    const int nbins = 2 * c->K;
    c->marg_valid = false;
    c->mspec_valid = false;            // (draws made ahead belong to the rows this pass replaces)
    // automatic: the one-collective form sends 3K rows instead of 2K -- 0.55 MB more at D = 64, K = 32 (a few us of wire) against a whole
    // latency-bound collective in the middle of the sort chain; at D = 256 the extra K rows are 8.4 MB (~80 us): the classic form stays
    const bool one_auto = c->packed_stride <= 4096;
    const bool one_coll = with_reset && comm_attached(c) && (c->opt_one_collective < 0 ? one_auto : c->opt_one_collective != 0);      // (both priors since round 5)
    c->last_pass_one_collective = one_coll;
    if (c->opt_timing & 2) HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    if (idx) {
        c->h_sel.assign(nbins, 0);
        for (int j = 0; j < n_idx; ++j) {
            if (idx[j] < 1 || idx[j] > c->K) return fail(c, DPMM_EINVAL, "cluster index out of range");
            c->h_sel[2 * (idx[j] - 1)] = 1;
            c->h_sel[2 * (idx[j] - 1) + 1] = 1;
        }
        if (int rc = ensure_pinned(c, nbins + 8)) return rc;
        HIPCHK(c, sync_stream(c, c->stream));
        memcpy(c->h_pin, c->h_sel.data(), nbins);
        HIPCHK(c, launch_copy_bytes(c->sb.bin_sel, c->h_pin, nbins, c->stream));
        c->sel_all_ones = 0;
    } else if (with_reset && c->n > 0 && c->opt_derive) {
        // (the per-step pass writes the selection of its 2K bins itself: starts_step_kernel)
    } else if (c->sel_all_ones < nbins) {
        HIPCHK(c, hipMemsetAsync(c->sb.bin_sel, 1, c->sel_capacity, c->stream));      // stays valid until a subset pass overwrites it
        c->sel_all_ones = c->sel_capacity;
    }
    bool derive = false;
    StatsArgs a{};
    a.X = c->dX; a.ldx = c->ldx; a.n = c->n; a.D = c->D; a.nbins = nbins; a.chunk = c->chunk;
    a.max_items = (int)((c->n + c->chunk - 1) / c->chunk) + nbins;
    a.range_groups = c->opt_stats_groups;
    a.sb = c->sb; a.slabs = c->d_slabs; a.slab_stride = c->slab_stride; a.out = (one_coll && c->prior == DPMM_PRIOR_NIW) ? c->d_red : c->d_out; a.packed_stride = c->packed_stride; a.row_off = c->d_row_off; a.inv_off = c->d_inv_off;      // (a.out, NIW one-collective pass: the reduce kernel writes the 3K travelling rows itself)
    if (with_reset && c->n > 0) {
        // reset_bad_clusters! (local_clusters_actions.jl:501-516) on the device, four launches: histogram (+ running bin totals) ->
        // [occupancies summed over the ranks] -> flags + sub-labels of flagged clusters re-drawn + touched tiles re-counted -> scan + starts
        // -> scatter.  The flags live right behind the packed rows, so that rows + flags reach the master in one copy.
        // DPMM_OPT_CHAIN_FUSION bit 8 (round 6): no reset launch -- the histogram counts the reset ahead for the clusters that are one-sided in a
        // tile, the scan derives the flags and picks those counts for flagged clusters, the scatter applies the re-draw while it places
        // (measured, round 6: the launch it removes costs 18 us at N = 1e7 and 7 us at the 8-GPU shard size; the three kernels that take its work
        //  over grow by 6.5 + 4.3 + 9.2 us and 2.4 + 2.0 + 3.4 us -- no gain at either size, so the bit is OFF by default; it is value-neutral and
        //  tested (tests/test_gpu_derive.py).  Bit 8 alone applies from 4e6 points per shard, bit 32 at any size.)
        const bool fold_reset = (c->opt_chain & 8) != 0 && (c->n >= 4000000 || (c->opt_chain & 32) != 0) && nbins <= STEP_SPEC_MAX_BINS &&
                                c->sb.tile_spec != nullptr && c->sb.spec_bins != nullptr;
        HIPCHK(c, launch_step_hist(c->dbins, c->n, nbins, c->sb, c->stream, fold_reset ? 1 : 0, c->first, c->seed, reset_epoch));
        const long long *gc = nullptr;
        if (comm_attached(c) && !one_coll) {
            HIPCHK(c, launch_widen_counts(c->sb.fast_total, FAST_TOTAL_STRIDE, c->d_counts64, nbins, c->stream));
            if (int rc = comm_allreduce(c, c->d_counts64, nbins, /*kind=*/0)) return rc;
            gc = c->d_counts64;
        }
        uint8_t *flags = reinterpret_cast<uint8_t *>(c->d_out.get()) + sizeof(double) * (size_t)nbins * (size_t)c->packed_stride;
        // (one collective: this shard's own occupancies decide which clusters are reset speculatively; the verdict follows the all-reduce)
        if (!fold_reset) HIPCHK(c, launch_step_reset(c->dbins, c->n, c->first, nbins, c->sb, gc, flags, c->K, c->seed, reset_epoch, one_coll ? c->d_cside : nullptr, c->stream));
        // Statistics of the SMALLER sub-cluster only wherever no point entered or left the cluster since its cluster-level row was
        // cached (labels are tracked by the histogram); the other sub-cluster is cache - computed (derive_rows_kernel below)
        derive = c->opt_derive != 0;
        const int force_all = (c->cache_force || c->cache_K != c->K) ? 1 : 0;
        const StepReset rs{gc, flags, c->K, one_coll ? c->d_cside : nullptr, c->first, c->seed, reset_epoch};
        HIPCHK(c, launch_step_scan_scatter(c->dbins, a, derive ? 1 : 0, force_all, c->opt_chain & 1, fold_reset ? &rs : nullptr, c->stream));
        if (derive) { c->sel_all_ones = 0; c->cache_force = false; c->cache_K = c->K; }
    } else {
        if (c->n > 0) {
            HIPCHK(c, launch_sort_by_bin(c->dbins, c->n, nbins, c->sb, c->stream));
        } else {
            HIPCHK(c, hipMemsetAsync(c->sb.bin_total, 0, sizeof(int32_t) * nbins, c->stream));
        }
        if (with_reset && one_coll) {
            HIPCHK(c, hipMemsetAsync(c->d_cside, 0, (size_t)c->K, c->stream));      // a rank without points has no candidates and adds zeros
        } else if (with_reset) {       // a rank without points: its occupancies are zero, the flags come from the other ranks' counts
            const long long *gc = nullptr;
            if (comm_attached(c)) {
                HIPCHK(c, launch_widen_counts(c->sb.bin_total, 1, c->d_counts64, nbins, c->stream));
                if (int rc = comm_allreduce(c, c->d_counts64, nbins, /*kind=*/0)) return rc;
                gc = c->d_counts64;
            }
            uint8_t *flags = reinterpret_cast<uint8_t *>(c->d_out.get()) + sizeof(double) * (size_t)nbins * (size_t)c->packed_stride;
            HIPCHK(c, launch_bad_flags(c->sb.bin_total, gc, c->K, flags, c->stream));
        }
        HIPCHK(c, launch_sort_finish(c->dbins, a, c->stream));
    }
    c->have_perm = c->n > 0;
    c->perm_nbins = nbins;
    if (flags_sent) *flags_sent = false;
    if (one_coll) {
        uint8_t *flags = reinterpret_cast<uint8_t *>(c->d_out.get()) + sizeof(double) * (size_t)nbins * (size_t)c->packed_stride;
        const size_t nred = 3 * (size_t)c->K * (size_t)c->packed_stride;
        if (c->n > 0 && c->prior == DPMM_PRIOR_NIW) {
            if (derive) { a.mode = c->sb.cmode; a.cache = c->d_ccache; a.dirty = c->sb.cdirty; a.K = c->K; }
            a.cside = c->d_cside; a.zero2 = flags + c->K;
            HIPCHK(c, launch_niw_stats(a, c->stream));
        } else if (c->n > 0) {
            // Multinomial: the usual statistics + derivation of the speculatively reset labels into d_out, then the travelling rows from them
            if (c->x_sparse) HIPCHK(c, launch_mult_stats_sparse(a, sparse_args(c), c->stream));
            else if (c->x_u8) HIPCHK(c, launch_mult_stats_u8(a, c->dX8, c->ld8, c->stream));
            else HIPCHK(c, launch_mult_stats(a, c->stream));
            if (derive) HIPCHK(c, launch_derive_rows(c->d_out, c->d_ccache, c->sb.cmode, c->sb.cdirty, c->packed_stride, c->K, flags, nullptr, c->stream));
            HIPCHK(c, launch_onecoll_rows(c->d_out, c->d_red, c->packed_stride, c->K, c->d_cside, flags, c->stream));
        } else {
            HIPCHK(c, hipMemsetAsync(c->d_red, 0, sizeof(double) * nred, c->stream));
            HIPCHK(c, hipMemsetAsync(flags + c->K, 0, 2, c->stream));
        }
        // the one exchange of the sweep (update_suff_stats_posterior!, local_clusters_actions.jl:206-254; aggregate_suff_stats)
        if (int rc = comm_allreduce(c, c->d_red, nred, /*kind=*/1)) return rc;
        // (flags_to: the caller's pinned block -- the verdict rides in this launch; its "any" byte starts at 0: the kernel only sets it, and
        // nothing of the stream reads or writes the block before this kernel)
        if (flags_to) flags_to[c->K] = 0;
        HIPCHK(c, launch_niw_finalize_rows(c->d_red, c->d_out, c->packed_stride, c->K, c->d_cside, flags, flags_to, c->stream));
        if (flags_to && flags_sent) *flags_sent = true;
        // the undo of the candidates that are not bad touches labels only: queued by the caller BEHIND what the master is waiting for
        c->undo_pending = true;
        c->comm_bytes[0] = 0;
        if (c->opt_timing & 2) HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
        c->have_stats_ev = (c->opt_timing & 2) != 0;
        c->rows_full_K = c->K;
        return DPMM_OK;
    }
    // (flags_to: the caller's pinned block for the bad-cluster flags -- they ride in the derivation's launch when no collective follows it)
    const bool ride = derive && flags_to != nullptr && !comm_attached(c);
    const uint8_t *fsrc = reinterpret_cast<const uint8_t *>(c->d_out.get()) + sizeof(double) * (size_t)nbins * (size_t)c->packed_stride;
    if (c->prior == DPMM_PRIOR_NIW) {
        if (derive) {       // the reduce kernel derives the rows that were not computed (one launch and one round trip of the rows less)
            a.mode = c->sb.cmode; a.cache = c->d_ccache; a.dirty = c->sb.cdirty; a.K = c->K;
            a.flags_src = ride ? fsrc : nullptr; a.flags_dst = ride ? flags_to : nullptr;
        }
        HIPCHK(c, launch_niw_stats(a, c->stream));
    } else {
        if (c->x_sparse) HIPCHK(c, launch_mult_stats_sparse(a, sparse_args(c), c->stream));
        else if (c->x_u8) HIPCHK(c, launch_mult_stats_u8(a, c->dX8, c->ld8, c->stream));
        else HIPCHK(c, launch_mult_stats(a, c->stream));
        if (derive) HIPCHK(c, launch_derive_rows(c->d_out, c->d_ccache, c->sb.cmode, c->sb.cdirty, c->packed_stride, c->K, fsrc, ride ? flags_to : nullptr, c->stream));
    }
    if (ride && flags_sent) *flags_sent = true;
    if (comm_attached(c)) {
        // the one exchange of the sweep: elementwise sum of the per-worker statistics (update_suff_stats_posterior!,
        // local_clusters_actions.jl:206-254; aggregate_suff_stats); N counts travel as Float64 integers (exact below 2^53)
        if (int rc = comm_allreduce(c, c->d_out, (size_t)nbins * (size_t)c->packed_stride, /*kind=*/1)) return rc;
    }
    if (c->opt_timing & 2) HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
    c->have_stats_ev = (c->opt_timing & 2) != 0;
    c->rows_full_K = idx ? -1 : c->K;           // (a subset pass zeroes the rows it was not asked for)
    return DPMM_OK;
}

int dpmm_bin_counts(dpmm_ctx *c, int64_t *counts) {
    if (!c || !counts) return DPMM_EINVAL;
    if (!c->have_points || !c->have_labels || c->K < 1) return fail(c, DPMM_ESTATE, "bin counts need points, labels and parameters (K)");
    HIPCHK(c, hipSetDevice(c->device));
    const int nbins = 2 * c->K;
    if (c->n == 0) { for (int b = 0; b < nbins; ++b) counts[b] = 0; return DPMM_OK; }
    if (int rc = ensure_pinned(c, sizeof(int32_t) * nbins)) return rc;
    HIPCHK(c, launch_sort_by_bin(c->dbins, c->n, nbins, c->sb, c->stream));      // hist + scan -> bin_total
    HIPCHK(c, launch_copy_bytes(c->h_pin, c->sb.bin_total, sizeof(int32_t) * nbins, c->stream));
    HIPCHK(c, sync_stream(c, c->stream));
    const int32_t *h = reinterpret_cast<const int32_t *>(c->h_pin.get());
    for (int b = 0; b < nbins; ++b) counts[b] = h[b];
    return DPMM_OK;
}

int dpmm_suffstats_packed_device(dpmm_ctx *c, const int64_t *idx, int n_idx, double *d_out) {
    if (!c || !d_out) return DPMM_EINVAL;
    if (int rc = run_stats(c, idx, n_idx)) return rc;
    HIPCHK(c, hipMemcpyAsync(d_out, c->d_out, sizeof(double) * 2 * c->K * (size_t)c->packed_stride, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, sync_stream(c, c->stream));
    return DPMM_OK;
}

// statistics (summed over the ranks when a communicator is attached) -> pinned host memory the caller reads in place
int dpmm_suffstats_host(dpmm_ctx *c, const int64_t *idx, int n_idx, const double **packed) {
    if (!c || !packed) return DPMM_EINVAL;
    const size_t out_bytes = sizeof(double) * 2 * (size_t)std::max(c->K, 1) * (size_t)c->packed_stride;
    if (int rc = ensure_out(c, out_bytes + DPMM_MAX_CLUSTERS + 64)) return rc;
    if (int rc = run_stats(c, idx, n_idx)) return rc;
    HIPCHK(c, launch_copy_bytes(c->h_out, c->d_out, out_bytes, c->stream));
    HIPCHK(c, sync_stream(c, c->stream));
    *packed = reinterpret_cast<const double *>(c->h_out.get());
    return DPMM_OK;
}

static int mult_marginals_launch(dpmm_ctx *c);
int dpmm_step_stats(dpmm_ctx *c, uint32_t reset_epoch, const double **packed, const uint8_t **bad) {
    if (!c || !packed || !bad) return DPMM_EINVAL;
    const size_t out_bytes = sizeof(double) * 2 * (size_t)std::max(c->K, 1) * (size_t)c->packed_stride;
    if (int rc = ensure_out(c, out_bytes + DPMM_MAX_CLUSTERS + 64)) return rc;
    // (a step that will deliver the rows late lets the flags ride to the pinned block with the kernel that derives the rows: one copy fewer)
    const bool maybe_late = c->rows_on_demand && c->marg_req && c->opt_mult_draws_ahead && c->mdraw_seen && c->draws_on_device && c->d_raw2;
    bool flags_sent = false;
    if (int rc = run_stats(c, nullptr, 0, true, reset_epoch, maybe_late ? reinterpret_cast<uint8_t *>(c->h_out + out_bytes) : nullptr, &flags_sent)) return rc;
    if (c->marg_req) if (int rc = mult_marginals_launch(c)) return rc;       // the master's log-marginals ride behind the statistics: one wait
    const bool with_marg = c->marg_valid && c->marg_K == c->K;            // the device master is running (the host asked for the log-marginals)
    const bool ahead = with_marg && c->opt_mult_draws_ahead && c->mdraw_seen && c->draws_on_device && c->rows_full_K == c->K && c->d_raw2 &&
                       (!c->marg_req_outlier || c->mult_has_alpha1);
    const bool late = ahead && c->rows_on_demand;       // the caller reads the rows through dpmm_mult_master_rows_wait only: flags now, rows behind the draws
    c->rows_late = false;
    if (late) { if (!flags_sent) HIPCHK(c, launch_copy_bytes(c->h_out + out_bytes, reinterpret_cast<const uint8_t *>(c->d_out.get()) + out_bytes, (size_t)c->K + 1, c->stream)); }
    else HIPCHK(c, launch_copy_bytes(c->h_out, c->d_out, out_bytes + (size_t)c->K + 1, c->stream));      // rows | flags
    if (int rc = flush_undo(c)) return rc;
    // Multinomial device master: the next Dirichlet draws + their hand-over images go out NOW, behind an event the host waits for instead of
    // the stream -- they run while it decides splits and merges (a quiet step then only uploads the weights; 24 us of kernels off the path)
    if (ahead) {
        if (!c->ev_rows) HIPCHK(c, hipEventCreateWithFlags(&c->ev_rows, hipEventDisableTiming));
        HIPCHK(c, hipEventRecord(c->ev_rows, c->stream));
        const int K = c->K;
        const uint32_t epoch = c->mdraw_epoch + 1;
        HIPCHK(c, launch_mult_dirichlet(c->d_out, c->packed_stride, c->d_malpha, c->mult_has_alpha1 ? c->d_malpha + c->ldx : nullptr, c->marg_req_outlier, c->D, c->ldx,
                                        K, c->seed, epoch, c->d_raw2, c->stream));
        c->rp2_current = !(c->x_u8 || c->x_bf16_exact || c->x_sparse);                 // (only the Float32 sweep kernel reads that image)
        if (c->rp2_current) HIPCHK(c, launch_mult_pack(c->d_raw2, c->d_Rp2, 3 * K, c->ldx, c->stream));
        if (c->x_sparse) if (int rc = pack_sparse_image(c, c->d_raw2, c->d_Rp2, K)) return rc;
        if (c->x_u8) HIPCHK(c, launch_mult_pack_u8(c->d_raw2, c->d_Lp16_2, 3 * K, c->ldx, c->ld8, c->stream));
        else if (c->x_bf16_exact) HIPCHK(c, launch_mult_pack_bf16(c->d_raw2, c->d_Lp16_2, 3 * K, c->ldx, c->stream));
        c->mspec_valid = true; c->mspec_epoch = epoch; c->mspec_K = K; c->mspec_outlier = c->marg_req_outlier;
        if (late) {
            // (on the same stream, behind the draws.  A second stream was measured twice and is no faster: beside the Dirichlet kernel the copy
            //  slows that kernel down by what the copy takes, behind the draws it shares the PCIe link with the upload of the next weights.
            //  No event of its own either: dpmm_mult_master_rows_wait is rare and waits for the stream)
            HIPCHK(c, launch_copy_bytes(c->h_out, c->d_out, out_bytes, c->stream));
            c->rows_late = true;
        }
        HIPCHK(c, sync_event(c, c->ev_rows));
        c->sync_gen += 1;                  // (the weights' copy of this step was queued long before ev_rows)
        c->marg_behind_ev = true;
    } else {
        HIPCHK(c, sync_stream(c, c->stream));
    }
    *packed = reinterpret_cast<const double *>(c->h_out.get());
    *bad = reinterpret_cast<const uint8_t *>(c->h_out + out_bytes);
    return DPMM_OK;
}

// ---- the master's dense maths on the device --------------------------------------------------------------------------------
static inline int master_pinned(dpmm_ctx *c, size_t bytes) { return grow(c, c->h_master, bytes, "dpmm_niw_master", "pinned block of the device master", (size_t)1 << 16); }
// the main stream waits for draws launched ahead on stream2 (before anything that writes what they read or reads what they write)
static int spec_join(dpmm_ctx *c) {
    if (c->spec_inflight) {
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_spec, 0));
        c->spec_inflight = false;
    }
    if (c->apairs_inflight) {             // (the pair job reads the stored rows a posterior pass is about to replace)
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_pairs, 0));
        c->apairs_inflight = false;
    }
    return DPMM_OK;
}
// ... and for the normals generated ahead (before a draw on the main stream: it uses them, or writes the buffer they are written to)
static int noise_join(dpmm_ctx *c) {
    if (c->noise_inflight) {
        // (a hipEventQuery in place of this barrier packet was tried: right after the record it reported the event's PREVIOUS completion
        // now and then -- draws from unwritten normals, caught by the moment test)
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_noise, 0));
        c->noise_inflight = false;
    }
    return DPMM_OK;
}
// the deferred launch of the normals of the next draws (requested by dpmm_niw_master_draw): into the draw buffer that is NOT in use
static int noise_flush(dpmm_ctx *c) {
    if (!c->noise_pending) return DPMM_OK;
    c->noise_pending = false;
    HIPCHK(c, launch_niw_master_noise(c->ma, c->noise_pend_nmat, c->noise_pend_epoch, c->d_Y[c->draw_cur ^ 1], c->stream2));
    HIPCHK(c, hipEventRecord(c->ev_noise, c->stream2));
    c->noise_inflight = true; c->noise_valid = true; c->noise_epoch = c->noise_pend_epoch; c->noise_nmat = c->noise_pend_nmat; c->noise_buf = c->draw_cur ^ 1;
    return DPMM_OK;
}
// the normals of the draws of `epoch` for K clusters are in d_Y[buf] (generated ahead on stream2)
static bool noise_ready(const dpmm_ctx *c, uint32_t epoch, int K, int buf) {
    return c->noise_valid && c->noise_epoch == epoch && 3 * K <= c->noise_nmat && c->noise_buf == buf;
}
// `data` [n] -> the device list `dst` (stream-ordered on the main stream; nothing is sent when the list is the one already there)
// The copy goes through a ring of pinned staging buffers and the library's own copy kernel, like every per-step transfer: on the test
// boxes hipMemcpyAsync takes the copy-engine path, which was seen to sit in a stream for 0.7 ms (rocprofv3: `__amd_rocclr_copyBuffer`).
// A staging slot is reused four changes later; every caller waits for its stream at least once per change.
static int device_list(dpmm_ctx *c, int32_t *dst, std::vector<int32_t> &shadow, const int32_t *data, size_t n, hipStream_t st = nullptr) {
    if (shadow.size() == n && (n == 0 || memcmp(shadow.data(), data, sizeof(int32_t) * n) == 0)) return DPMM_OK;
    shadow.assign(data, data + n);
    if (n == 0) return DPMM_OK;
    const size_t bytes = sizeof(int32_t) * n;
    PinBuf<int32_t> &slot = c->h_list[c->h_list_next];
    c->h_list_next = (c->h_list_next + 1) % 4;
    if (bytes > slot.bytes) if (int rc = regrow(c, slot, bytes, "device master", "pinned staging of an index list", 4096)) return rc;      // (no wait: see above)
    memcpy(slot, data, bytes);
    HIPCHK(c, launch_copy_bytes(dst, slot, bytes, st ? st : c->stream));
    return DPMM_OK;
}
// device storage for `slots` slots (posterior state, kept across growth) and K clusters (draw scratch)
static int master_capacity(dpmm_ctx *c, int slots, int K) {
    const size_t DP = (size_t)c->ma.DP, stride = (size_t)c->packed_stride;
    if (slots > c->master_slots) {
        int ns = std::max(8, c->master_slots);
        while (ns < slots) ns *= 2;
        ns = std::min(ns, DPMM_MAX_CLUSTERS);
        HIPCHK(c, sync_stream(c, c->stream));
        if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
        c->spec_valid = false; c->noise_valid = false; c->apairs_valid = false;
        DevBuf<double> fac, mean, kap, nu, rows;      // beside the old ones, whose contents they take over
        HIPCHK(c, fac.alloc(sizeof(double) * 3 * ns * DP * DP));
        HIPCHK(c, mean.alloc(sizeof(double) * 3 * ns * DP));
        HIPCHK(c, kap.alloc(sizeof(double) * 3 * ns));
        HIPCHK(c, nu.alloc(sizeof(double) * 3 * ns));
        HIPCHK(c, rows.alloc(sizeof(double) * 2 * ns * stride));
        if (c->master_slots > 0) {
            const size_t os = (size_t)c->master_slots;
            HIPCHK(c, hipMemcpy(fac, c->ma.fac, sizeof(double) * 3 * os * DP * DP, hipMemcpyDeviceToDevice));
            HIPCHK(c, hipMemcpy(mean, c->ma.mean, sizeof(double) * 3 * os * DP, hipMemcpyDeviceToDevice));
            HIPCHK(c, hipMemcpy(kap, c->ma.kap, sizeof(double) * 3 * os, hipMemcpyDeviceToDevice));
            HIPCHK(c, hipMemcpy(nu, c->ma.nu, sizeof(double) * 3 * os, hipMemcpyDeviceToDevice));
            HIPCHK(c, hipMemcpy(rows, c->ma.rows_store, sizeof(double) * 2 * os * stride, hipMemcpyDeviceToDevice));
        }
        auto &m = c->master_mem;
        m.fac = std::move(fac); m.mean = std::move(mean); m.kap = std::move(kap); m.nu = std::move(nu); m.rows_store = std::move(rows);
        c->ma.fac = m.fac; c->ma.mean = m.mean; c->ma.kap = m.kap; c->ma.nu = m.nu; c->ma.rows_store = m.rows_store;
        c->master_slots = ns;
    }
    if (K > c->master_K) {
        int nk = std::max(8, c->master_K);
        while (nk < K) nk *= 2;
        nk = std::min(nk, DPMM_MAX_CLUSTERS);
        HIPCHK(c, sync_stream(c, c->stream));
        if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
        c->spec_valid = false; c->noise_valid = false; c->apairs_valid = false;
        for (int i = 0; i < 2; ++i) {
            HIPCHK(c, c->d_Y[i].alloc(sizeof(double) * 3 * nk * DP * DP));
            HIPCHK(c, c->d_ld_sigma[i].alloc(sizeof(float) * 3 * nk));
            HIPCHK(c, c->d_mu_draw[i].alloc(sizeof(float) * 3 * nk * DP));
        }
        c->draws_on_device = false;
        c->master_K = nk;
    }
    return DPMM_OK;
}

int dpmm_niw_master_setup(dpmm_ctx *c, double kappa, double nu, const double *m, const double *psi) {
    if (!c || !m || !psi) return DPMM_EINVAL;
    if (c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, "the device master exists for the NIW prior only");
    if (c->D > DPMM_MASTER_MAXD) return fail(c, DPMM_ELIMIT, "D exceeds the device master's limit");
    HIPCHK(c, hipSetDevice(c->device));
    const int D = c->D;
    const size_t T = (size_t)D * (D + 1) / 2;
    std::vector<double> lo(T);
    for (int a = 0; a < D; ++a)
        for (int b = 0; b <= a; ++b) lo[(size_t)a * (a + 1) / 2 + b] = 0.5 * (psi[(size_t)a * D + b] + psi[(size_t)b * D + a]);
    HIPCHK(c, sync_stream(c, c->stream));
    if (!c->d_m0) HIPCHK(c, c->d_m0.alloc(sizeof(double) * D));
    if (!c->d_psi_lo) HIPCHK(c, c->d_psi_lo.alloc(sizeof(double) * T));
    HIPCHK(c, hipMemcpy(c->d_m0, m, sizeof(double) * D, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_psi_lo, lo.data(), sizeof(double) * T, hipMemcpyHostToDevice));
    c->ma.D = D; c->ma.DP = 16 * ((D + 15) / 16); c->ma.packed_stride = c->packed_stride;
    c->ma.kappa0 = kappa; c->ma.nu0 = nu; c->ma.m0 = c->d_m0; c->ma.psi_lo = c->d_psi_lo; c->ma.seed = c->seed;
    if (!c->h_draw) HIPCHK(c, c->h_draw.alloc(sizeof(float) * 3 * DPMM_MAX_CLUSTERS));
    if (!c->stream2) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_master, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_spec, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_noise, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_pairs, hipEventDisableTiming));
        HIPCHK(c, c->d_jobs.alloc(sizeof(int32_t) * 2 * DPMM_MAX_CLUSTERS));
        HIPCHK(c, c->d_dslots.alloc(sizeof(int32_t) * DPMM_MAX_CLUSTERS));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream2));
    c->spec_inflight = false; c->spec_valid = false; c->noise_inflight = false; c->noise_valid = false; c->noise_pending = false;
    c->apairs_inflight = false; c->apairs_valid = false;
    c->master = true;
    return DPMM_OK;
}

int dpmm_step_stats_device(dpmm_ctx *c, uint32_t reset_epoch, const uint8_t **bad) {
    if (!c || !bad) return DPMM_EINVAL;
    if (!c->master) return fail(c, DPMM_ESTATE, "dpmm_niw_master_setup first");
    const size_t out_bytes = sizeof(double) * 2 * (size_t)std::max(c->K, 1) * (size_t)c->packed_stride;
    if (int rc = ensure_out(c, DPMM_MAX_CLUSTERS + 64)) return rc;
    if (int rc = run_stats(c, nullptr, 0, true, reset_epoch)) return rc;
    HIPCHK(c, launch_copy_bytes(c->h_out, reinterpret_cast<const uint8_t *>(c->d_out.get()) + out_bytes, (size_t)c->K + 1, c->stream));
    if (int rc = flush_undo(c)) return rc;
    HIPCHK(c, sync_stream(c, c->stream));
    *bad = reinterpret_cast<const uint8_t *>(c->h_out.get());
    return DPMM_OK;
}

static const uint64_t MASTER_MARK = 0x7ff8dead0000beefull;
static bool master_records_marked(const double *sm, int64_t nrec) {
    const volatile uint64_t *w = reinterpret_cast<const volatile uint64_t *>(sm);
    for (int64_t r = nrec - 1; r >= 0; --r)           // (from the back: the last workgroups of the launch finish last)
        for (int e = 0; e < 5; ++e) if (w[r * DPMM_MASTER_NSCALARS + e] == MASTER_MARK) return true;
    return false;
}
static bool master_marks_left(const double *sm, int K) { return master_records_marked(sm, 3 * (int64_t)K); }
static void master_mark_records(double *sm, int64_t nrec) {
    for (int64_t r = 0; r < nrec; ++r)
        for (int e = 0; e < 5; ++e) std::memcpy(&sm[r * DPMM_MASTER_NSCALARS + e], &MASTER_MARK, 8);
}
// The wait of dpmm_step_master_device WITHOUT an event (DPMM_OPT_MASTER_POLL, round 6).  The posterior workgroups store their five scalars per
// distribution straight into pinned host memory; every record starts out as MASTER_MARK (a NaN payload no kernel produces), so "no mark left"
// IS "the posteriors' results are on the host" -- the witness of rounds 3-5 promoted to the wait itself.  What it buys: no event record sits
// between the posteriors and the draws launched ahead behind them (a barrier packet with a completion signal: 6 us of stream time at
// N = 1e7, 10 us at the 8-GPU shard size where the second stream's normals join there too), and the host sees the records when they land
// instead of when the runtime has processed the signal.  Everything an EARLIER kernel of the stream wrote to pinned memory (the bad-cluster
// flags) is complete by then: a kernel starts after its predecessor's end-of-kernel release.  The loop keeps the watchdog's contract (a wait
// behind an enqueued collective is armed; an abort ends it) and asks the stream once a millisecond whether it failed or drained.
static int wait_master_records(dpmm_ctx *c, const double *sm, int64_t nrec, const double *pr, int64_t npr) {
    const bool armed = c->watchdog && c->coll_pending;
    if (armed) wd_arm(c);
    int rc = DPMM_OK;
    const auto t0 = std::chrono::steady_clock::now();
    auto next_query = t0 + std::chrono::milliseconds(1);
    std::chrono::steady_clock::time_point drained{};
    bool is_drained = false;
    for (uint64_t spin = 0;; ++spin) {
        if (!master_records_marked(sm, nrec) && !(npr > 0 && master_records_marked(pr, npr))) break;
        __builtin_ia32_pause();
        if ((spin & 63u) != 63u) continue;
        if (c->comm_aborted.load(std::memory_order_relaxed)) break;                         // (reported by wd_disarm below)
        const auto now = std::chrono::steady_clock::now();
        if (now < next_query) continue;
        next_query = now + std::chrono::milliseconds(1);
        const hipError_t q = hipStreamQuery(c->stream);
        if (q == hipSuccess) {       // the stream is empty and records are still marked: stores in flight (seen in rounds 3-5 behind an event wait) -- or never written
            if (!is_drained) { is_drained = true; drained = now; ++c->dbg_early_wait; }
            else if (now - drained > std::chrono::seconds(5)) { rc = fail(c, DPMM_EHIP, "posterior records missing 5 s after the stream drained"); break; }
        } else if (q != hipErrorNotReady) { c->err = std::string("hipStreamQuery while waiting for the posteriors: ") + hipGetErrorString(q); rc = DPMM_EHIP; break; }
    }
    if (armed && wd_disarm(c)) {
        c->err = "collective timed out: a peer rank is gone or stuck (communicator aborted after DPMM_OPT_COMM_TIMEOUT_MS)";
        return DPMM_ECOMM;
    }
    if (c->comm_aborted.load(std::memory_order_relaxed) && rc == DPMM_OK && master_records_marked(sm, nrec)) return fail(c, DPMM_ECOMM, "communicator aborted");
    return rc;
}

int dpmm_debug_set_prelaunch_hook(void (*fn)(void *), void *arg) {
    dpmm::g_prelaunch_arg = arg;
    dpmm::g_prelaunch = fn;
    return DPMM_OK;
}

int dpmm_debug_counters(dpmm_ctx *c, int64_t *out, int n) {
    if (!c || !out || n < 1) return DPMM_EINVAL;
    for (int i = 0; i < n; ++i) out[i] = 0;
    out[0] = c->dbg_early_wait;
    return DPMM_OK;
}

int dpmm_debug_sort_tables(dpmm_ctx *c, int32_t *perm, int32_t *bin_total, int32_t *bin_start, int32_t *perm_total) {
    if (!c || !perm || !bin_total || !bin_start || !perm_total) return DPMM_EINVAL;
    if (!c->have_perm || c->K < 1) return fail(c, DPMM_ESTATE, "no statistics pass has sorted the points yet");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(perm, c->sb.perm, sizeof(int32_t) * (size_t)c->n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(bin_total, c->sb.bin_total, sizeof(int32_t) * 2 * (size_t)c->K, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(bin_start, c->sb.bin_start, sizeof(int32_t) * (2 * (size_t)c->K + 1), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(perm_total, c->sb.perm_total, sizeof(int32_t), hipMemcpyDeviceToHost));
    return DPMM_OK;
}

int dpmm_step_master_device(dpmm_ctx *c, uint32_t reset_epoch, const int32_t *slots, uint32_t draw_epoch, const uint8_t **bad, const double **small) {
    if (!c || !slots || !bad || !small) return DPMM_EINVAL;
    if (!c->master) return fail(c, DPMM_ESTATE, "dpmm_niw_master_setup first");
    const int K = c->K;
    if (K < 1) return fail(c, DPMM_ESTATE, "no clusters");
    HIPCHK(c, hipSetDevice(c->device));
    int top = 0;
    for (int k = 0; k < K; ++k) {
        if (slots[k] < 0 || slots[k] >= DPMM_MAX_CLUSTERS) return fail(c, DPMM_EINVAL, "slot out of range");
        top = std::max(top, slots[k] + 1);
    }
    if (int rc = noise_flush(c)) return rc;
    if (int rc = master_capacity(c, top, draw_epoch ? K : 0)) return rc;
    if (int rc = spec_join(c)) return rc;                  // unused early draws of the last call still read the factors
    c->spec_valid = false;
    const size_t out_bytes = sizeof(double) * 2 * (size_t)K * (size_t)c->packed_stride;
    if (int rc = ensure_out(c, DPMM_MAX_CLUSTERS + 64)) return rc;
    const size_t jobs_bytes = (sizeof(int32_t) * 2 * (size_t)K + 63) & ~(size_t)63;
    if (int rc = master_pinned(c, jobs_bytes + sizeof(double) * 3 * DPMM_MASTER_NSCALARS * (size_t)K)) return rc;
    // every user of the pinned block waits for its kernels before returning, so it is free here; no wait -- the sweep is still in flight
    std::vector<int32_t> jobs(2 * (size_t)K);
    for (int k = 0; k < K; ++k) { jobs[2 * k] = k; jobs[2 * k + 1] = slots[k]; }
    if (int rc = device_list(c, c->d_jobs, c->jobs_shadow, jobs.data(), jobs.size())) return rc;
    if (draw_epoch) if (int rc = device_list(c, c->d_dslots, c->dslots_shadow, slots, (size_t)K)) return rc;
    for (int32_t sl : c->apairs_req) if (sl >= top) { c->apairs_req.clear(); break; }      // (a pair of a slot this pass does not cover: no job)
    const int napairs = (int)(c->apairs_req.size() / 2);
    c->apairs_valid = false;
    bool fuse_pairs = true;
    if (napairs > 0) {
        if ((size_t)napairs > c->apairs_cap) {
            HIPCHK(c, sync_stream(c, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream2));
            const size_t cap = grow_capacity((size_t)napairs, 64);
            c->apairs_cap = 0; c->apairs_shadow.clear();
            HIPCHK(c, c->d_apairs.alloc(sizeof(int32_t) * 2 * cap));
            HIPCHK(c, c->h_apairs.alloc(sizeof(double) * DPMM_MASTER_NSCALARS * cap));
            c->apairs_cap = cap;
        }
        if (c->ma.DP > 128 && (size_t)napairs > c->pair_cap) {      // scratch matrices of the large-D pair kernels
            HIPCHK(c, sync_stream(c, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream2));
            const size_t cap = grow_capacity((size_t)napairs, 64);
            c->pair_cap = 0;
            HIPCHK(c, c->d_pairs.alloc(sizeof(double) * cap * (size_t)c->ma.DP * (size_t)c->ma.DP));
            c->pair_cap = cap;
        }
        // (on the second stream, where the pair job runs: the list changes with the merge gates, and a copy on the main stream would sit
        // between the sweep and the statistics kernels)
        if (niw_master_can_fuse_pairs(c->ma)) {
            // D <= 128: the pair jobs ride in the posteriors' launch (below) and name CLUSTERS of this pass
            std::vector<int32_t> inv((size_t)top, -1), kp(c->apairs_req.size());
            for (int k = 0; k < K; ++k) inv[slots[k]] = k;
            for (size_t i = 0; i < kp.size(); ++i) {
                kp[i] = inv[c->apairs_req[i]];
                if (kp[i] < 0) { fuse_pairs = false; break; }
            }
            if (fuse_pairs) {
                // The fused pair jobs read their two cluster indices straight from pinned host memory (round 6): the list changes whenever a merge
                // gate opens or closes (a bad-cluster reset closes one: most steps of the bench chain), and the copy launch that brought it to the
                // device sat on the main stream between the sweep and the statistics kernels (5 us).  Two buffers take turns: the launch that read
                // the other one has been waited for (its records were) before a new list is written.
                if (c->opt_chain & 4) {
                    if (!(c->apairs_shadow.size() == kp.size() && memcmp(c->apairs_shadow.data(), kp.data(), sizeof(int32_t) * kp.size()) == 0) || !c->apairs_pinned_cur) {
                        c->apairs_shadow.assign(kp.begin(), kp.end());
                        c->apairs_pin_flip ^= 1;
                        PinBuf<int32_t> &buf = c->h_apairs_list[c->apairs_pin_flip];
                        const size_t need = sizeof(int32_t) * kp.size();
                        if (need > buf.bytes) if (int rc = regrow(c, buf, need, "dpmm_step_master_device", "pinned list of the fused pair jobs", sizeof(int32_t) * 2048)) return rc;      // (no wait: see above)
                        memcpy(buf, kp.data(), need);
                        c->apairs_pinned_cur = buf;
                    }
                } else {
                    if (c->apairs_pinned_cur) { c->apairs_shadow.clear(); c->apairs_pinned_cur = nullptr; }      // (the shadow described the pinned list, not d_apairs)
                    if (int rc = device_list(c, c->d_apairs, c->apairs_shadow, kp.data(), kp.size())) return rc;
                }
            }
        } else fuse_pairs = false;
        if (!fuse_pairs) {
            if (c->apairs_pinned_cur) { c->apairs_shadow.clear(); c->apairs_pinned_cur = nullptr; }
            if (int rc = device_list(c, c->d_apairs, c->apairs_shadow, c->apairs_req.data(), c->apairs_req.size(), c->stream2)) return rc;
        }
    } else fuse_pairs = false;
    double *sm = reinterpret_cast<double *>(c->h_master + jobs_bytes);
    // Witness of the event wait below: every scalar record the posteriors write starts out as a marker no kernel produces (a NaN with a
    // payload; the kernels' own NaN is the plain quiet one).  A record still carrying it after the wait means the wait returned before
    // the kernels' stores reached host memory: counted (dpmm_debug_counters) and waited out.
    master_mark_records(sm, 3 * (int64_t)K);
    const bool poll = c->opt_master_poll != 0;
    bool flags_sent = false;
    if (int rc = run_stats(c, nullptr, 0, true, reset_epoch, reinterpret_cast<uint8_t *>(c->h_out.get()), &flags_sent)) return rc;
    if (!flags_sent) HIPCHK(c, launch_copy_bytes(c->h_out, reinterpret_cast<const uint8_t *>(c->d_out.get()) + out_bytes, (size_t)K + 1, c->stream));
    // DPMM_OPT_CHAIN_FUSION bit 16 (D <= 128, draws launched ahead): the normals of those draws are generated by extra workgroups of the
    // posteriors' launch (niw_post_both_kernel) -- no kernel beside the sweep on the second stream, no cross-stream wait in front of the draws
    const bool noise_in_post = draw_epoch != 0 && (c->opt_chain & 16) != 0 && niw_master_can_fuse_pairs(c->ma);
    bool normals_by_post = false;
    if (noise_in_post) {
        if (int rc = noise_join(c)) return rc;                 // (a kernel of the other scheme still writing that buffer: rare -- the option was just switched)
        c->noise_valid = false;
    }
    if ((napairs > 0 && fuse_pairs) || noise_in_post) {
        // posteriors + the pooled pair log-determinants the master may ask for (dpmm_niw_master_pairs_ahead) in ONE launch: the pairs need
        // the rows of this pass only.  (On the second stream behind the posteriors they reached the host 12 + 26 us later.)
        const int nfp = fuse_pairs ? napairs : 0;
        if (poll && nfp > 0) master_mark_records(c->h_apairs, nfp);      // (nobody reads the pair records between two passes: dpmm_niw_master_pairs copies them out)
        HIPCHK(c, launch_niw_master_posterior_pairs(c->ma, c->d_jobs, K, c->d_out, sm, ((c->opt_chain & 4) && c->apairs_pinned_cur) ? c->apairs_pinned_cur : c->d_apairs, nfp, c->h_apairs, c->stream,
                                                    noise_in_post ? 3 * K : 0, draw_epoch, noise_in_post ? c->d_Y[c->draw_cur ^ 1] : nullptr));
        normals_by_post = noise_in_post;
    } else HIPCHK(c, launch_niw_master_posterior(c->ma, c->d_jobs, K, c->d_out, sm, c->stream));
    if (napairs > 0 && fuse_pairs) {
        c->apairs_index.clear();
        for (int p = 0; p < napairs; ++p) c->apairs_index[((uint32_t)c->apairs_req[2 * p] << 16) | (uint32_t)c->apairs_req[2 * p + 1]] = p;
        c->apairs_dirty.assign((size_t)c->master_slots, 0);
        c->apairs_inflight = false; c->apairs_valid = true;      // (the host waits for ev_master below: the records are there when it returns)
        c->apairs_req.clear();
    }
    const bool fused_pairs_launched = napairs > 0 && fuse_pairs;
    const bool need_event = !poll || (napairs > 0 && !fuse_pairs);      // (the second stream's pair job waits for the posteriors through it)
    if (need_event) HIPCHK(c, hipEventRecord(c->ev_master, c->stream));
    if (napairs > 0 && !fuse_pairs) {
        // The pooled pair log-determinants the master may ask for after its split decisions (dpmm_niw_master_pairs_ahead): they need the
        // stored rows of this pass only, so they run on the second stream while the host works; dpmm_niw_master_pairs answers from
        // them when every pair it is asked for is among them and none of their slots got new statistics in between.
        HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_master, 0));
        HIPCHK(c, launch_niw_master_pairs(c->ma, c->d_apairs, napairs, c->d_pairs, c->h_apairs, c->stream2));
        HIPCHK(c, hipEventRecord(c->ev_pairs, c->stream2));
        c->apairs_index.clear();
        for (int p = 0; p < napairs; ++p) c->apairs_index[((uint32_t)c->apairs_req[2 * p] << 16) | (uint32_t)c->apairs_req[2 * p + 1]] = p;
        c->apairs_dirty.assign((size_t)c->master_slots, 0);
        c->apairs_inflight = true; c->apairs_valid = true;
        c->apairs_req.clear();
    }
    if (draw_epoch) {
        // The next parameter draws, launched now on the second stream: they need the posteriors only (not the weights, not the
        // master's split / merge decisions), so they run while the host works on the scalars this call returns.  If nothing changes
        // the cluster -> slot map until dpmm_niw_master_draw(draw_epoch, ...), that call finds them done and launches the hand-over alone.
        // (On the MAIN stream, right behind the posteriors and behind the event the host waits for: a hand-over across two streams costs
        // ~15 us of signalling each way -- posteriors -> draws -> pack took 26 + 14 + 27 + 17 + 10 us at the 8-GPU shard size, the gaps
        // being the two cross-stream waits.  The normals were generated on the second stream during the sweep: that event is long done.)
        const int32_t *hs = c->d_dslots;
        const bool have_normals = normals_by_post || noise_ready(c, draw_epoch, K, c->draw_cur ^ 1);
        if (int rc = noise_join(c)) return rc;             // (also when its normals are not the ones wanted: the kernel writes the buffer the draws go to)
        NiwMasterArgs ma = c->ma;
        ma.mu_draw = c->d_mu_draw[c->draw_cur ^ 1];
        HIPCHK(c, launch_niw_master_draw(ma, hs, K, draw_epoch, c->d_Y[c->draw_cur ^ 1], c->d_ld_sigma[c->draw_cur ^ 1], nullptr, nullptr,
                                         nullptr, nullptr, nullptr, nullptr, c->NB, nullptr, 1 | (have_normals ? 4 : 0), c->stream));
        c->noise_valid = false;
        c->spec_inflight = false; c->spec_valid = true; c->spec_epoch = draw_epoch;
        c->spec_slots.assign(slots, slots + K);
    }
    if (int rc = flush_undo(c)) return rc;      // (behind the posteriors, the event and the draws launched ahead)
    if (poll) { if (int rc = wait_master_records(c, sm, 3 * (int64_t)K, c->h_apairs, fused_pairs_launched ? napairs : 0)) return rc; }
    else HIPCHK(c, sync_event(c, c->ev_master));
    if (master_marks_left(sm, K)) {
        ++c->dbg_early_wait;
        const auto t0 = std::chrono::steady_clock::now();
        while (master_marks_left(sm, K)) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) return fail(c, DPMM_EHIP, "posterior records missing 5 s after the event wait returned");
            HIPCHK(c, sync_stream(c, c->stream));
        }
    }
    c->handover_inflight = false;          // (recorded behind the last hand-over kernel on the same stream)
    *bad = reinterpret_cast<const uint8_t *>(c->h_out.get());
    *small = sm;
    return DPMM_OK;
}

int dpmm_suffstats_device(dpmm_ctx *c, const int64_t *idx, int n_idx) {
    if (!c) return DPMM_EINVAL;
    if (!c->master) return fail(c, DPMM_ESTATE, "dpmm_niw_master_setup first");
    return run_stats(c, idx, n_idx);
}

int dpmm_niw_master_posterior(dpmm_ctx *c, const int64_t *clusters, const int32_t *slots, int n, const double **small) {
    if (!c || !slots || !small || n < 0) return DPMM_EINVAL;
    if (!c->master) return fail(c, DPMM_ESTATE, "dpmm_niw_master_setup first");
    if (n == 0) { *small = nullptr; return DPMM_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    int top = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t k = clusters ? clusters[i] : i + 1;
        if (k < 1 || k > c->K) return fail(c, DPMM_EINVAL, "cluster index out of range");
        if (slots[i] < 0 || slots[i] >= DPMM_MAX_CLUSTERS) return fail(c, DPMM_EINVAL, "slot out of range");
        top = std::max(top, slots[i] + 1);
    }
    if (int rc = master_capacity(c, top, 0)) return rc;
    if (int rc = spec_join(c)) return rc;
    c->spec_valid = false;                                 // some factors change: draws launched ahead are not the ones to use
    for (int i = 0; i < n; ++i) if ((size_t)slots[i] < c->apairs_dirty.size()) c->apairs_dirty[slots[i]] = 1;      // ... nor pooled pairs that involve these slots
    const size_t jobs_bytes = (sizeof(int32_t) * 2 * (size_t)n + 63) & ~(size_t)63;
    if (int rc = master_pinned(c, jobs_bytes + sizeof(double) * 3 * DPMM_MASTER_NSCALARS * (size_t)n)) return rc;
    HIPCHK(c, sync_stream(c, c->stream));            // nobody reads the pinned block any more
    std::vector<int32_t> jobs(2 * (size_t)n);
    for (int i = 0; i < n; ++i) { jobs[2 * i] = (int32_t)((clusters ? clusters[i] : i + 1) - 1); jobs[2 * i + 1] = slots[i]; }
    if (int rc = device_list(c, c->d_jobs, c->jobs_shadow, jobs.data(), jobs.size())) return rc;
    double *sm = reinterpret_cast<double *>(c->h_master + jobs_bytes);
    HIPCHK(c, launch_niw_master_posterior(c->ma, c->d_jobs, n, c->d_out, sm, c->stream));
    HIPCHK(c, sync_stream(c, c->stream));
    *small = sm;
    return DPMM_OK;
}

int dpmm_niw_master_draw(dpmm_ctx *c, uint32_t epoch, int K, const int32_t *slot_of_cluster, const float *lr, const float *w) {
    if (!c || !slot_of_cluster || !lr || !w) return DPMM_EINVAL;
    if (!c->master) return fail(c, DPMM_ESTATE, "dpmm_niw_master_setup first");
    if (int rc = check_K(c, K)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    for (int k = 0; k < K; ++k)
        if (slot_of_cluster[k] < 0 || slot_of_cluster[k] >= c->master_slots) return fail(c, DPMM_EINVAL, "slot without a posterior on the device");
    if (int rc = noise_flush(c)) return rc;
    if (int rc = ensure_capacity(c, K)) return rc;
    if (int rc = master_capacity(c, 0, K)) return rc;
    // small inputs through a pinned block of their own (the posterior's block may still be read by its caller)
    // lr / w through a pinned block of their own (h_draw; the shared staging h_pin belongs to calls that synchronise before they use it).
    // The previous hand-over kernel reads lr / w from this block: wait only if the host has not waited for anything behind it since
    // (in the engine's loop it has -- for the posteriors of the step -- and the stream now carries the draws launched ahead, which a
    // synchronise here would wait out: 27 us on the host's critical path at D = 64)
    if (c->handover_inflight) HIPCHK(c, sync_stream(c, c->stream));
    c->handover_inflight = true;
    float *hlr = reinterpret_cast<float *>(c->h_draw.get()), *hw = hlr + 2 * K;
    memcpy(hlr, lr, sizeof(float) * 2 * K);
    memcpy(hw, w, sizeof(float) * K);
    c->have_tail = c->opt_tail && c->D >= 4 && c->D % 4 == 0 && K > 1;
    // draws launched ahead by dpmm_step_master_device for this epoch and this cluster -> slot map: only the hand-over is left
    const bool ahead = c->spec_valid && c->spec_epoch == epoch && (int)c->spec_slots.size() == K &&
                       memcmp(c->spec_slots.data(), slot_of_cluster, sizeof(int32_t) * K) == 0;
    if (int rc = spec_join(c)) return rc;
    c->spec_valid = false;
    if (int rc = noise_join(c)) return rc;                 // (no-op when the draws launched ahead already waited for the normals)
    if (!ahead) if (int rc = device_list(c, c->d_dslots, c->dslots_shadow, slot_of_cluster, (size_t)K)) return rc;
    const int32_t *hs = c->d_dslots;
    c->draw_cur ^= 1;
    NiwMasterArgs ma = c->ma;
    ma.mu_draw = c->d_mu_draw[c->draw_cur];
    const bool normals = !ahead && noise_ready(c, epoch, K, c->draw_cur);       // (noise_join above made the main stream wait for them)
    c->predictive = false;              // (before the tables, as in set_params)
    // DPMM_OPT_CHAIN_FUSION bit 2: the hand-over partitioned by role, with the three-plane images in the same launch (no niw_b3_pack launch)
    const bool roles = (c->opt_chain & 2) != 0, b3_in_pack = roles && want_b3_images(c), pb_in_pack = b3_in_pack && want_pair_ball(c, K);
    if (pb_in_pack) c->sn2_tight = norm_tight(c);
    HIPCHK(c, launch_niw_master_draw(ma, hs, K, epoch, c->d_Y[c->draw_cur], c->d_ld_sigma[c->draw_cur], hlr, hw, c->d_Rp, c->d_mup, c->d_cst,
                                     c->have_tail ? c->d_tail : nullptr, c->NB, c->d_work, (ahead ? 2 : (normals ? 7 : 3)) | (roles ? 8 : 0) | (b3_in_pack ? 16 : 0) | (pb_in_pack ? 32 : 0) | ((pb_in_pack && c->sn2_tight) ? 64 : 0), c->stream));
    if (int rc = direction_tables(c, K, b3_in_pack, pb_in_pack)) return rc;
    // The normals of the NEXT draws (epoch + 1, a few clusters more than now for the splits in between) into the other buffer, on the
    // second stream: they depend on nothing the master decides, and run beside the sweep instead of in front of it.  Whoever draws
    // with another epoch, or for more clusters, generates its own.
    // (launched by noise_flush right AFTER the sweep kernel of this step: the launch and its event record would otherwise sit on the
    // host's critical path between the master's decisions and the sweep launch)
    c->noise_pending = c->opt_noise_ahead < 0 ? (c->D >= 128 || c->n < 4000000) : c->opt_noise_ahead != 0; c->noise_pend_epoch = epoch + 1; c->noise_pend_nmat = 3 * std::min(K + 4, c->master_K);
    if ((c->opt_chain & 16) && niw_master_can_fuse_pairs(c->ma)) c->noise_pending = false;      // (the posteriors' launch generates them: dpmm_step_master_device)
    c->work_zeroed = true;
    c->have_screen_prep = false;     // (the K > 64 far mask needs the raw factors: not built on this path; the tail screen is)
    c->K = K;
    c->have_params = true;
    c->predictive = false;
    c->draws_on_device = true;
    return DPMM_OK;
}

int dpmm_niw_master_pairs_ahead(dpmm_ctx *c, const int32_t *slots_i, const int32_t *slots_j, int n) {
    if (!c || n < 0 || (n > 0 && (!slots_i || !slots_j))) return DPMM_EINVAL;
    if (!c->master) return fail(c, DPMM_ESTATE, "dpmm_niw_master_setup first");
    c->apairs_req.clear();
    for (int i = 0; i < n; ++i) {
        if (slots_i[i] < 0 || slots_i[i] >= DPMM_MAX_CLUSTERS || slots_j[i] < 0 || slots_j[i] >= DPMM_MAX_CLUSTERS) { c->apairs_req.clear(); return fail(c, DPMM_EINVAL, "slot out of range"); }
        c->apairs_req.push_back(slots_i[i]); c->apairs_req.push_back(slots_j[i]);
    }
    return DPMM_OK;
}

int dpmm_niw_master_pairs(dpmm_ctx *c, const int32_t *slots_i, const int32_t *slots_j, int n, const double **small) {
    if (!c || !slots_i || !slots_j || !small || n < 0) return DPMM_EINVAL;
    if (!c->master) return fail(c, DPMM_ESTATE, "dpmm_niw_master_setup first");
    if (n == 0) { *small = nullptr; return DPMM_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    for (int i = 0; i < n; ++i)
        if (slots_i[i] < 0 || slots_i[i] >= c->master_slots || slots_j[i] < 0 || slots_j[i] >= c->master_slots) return fail(c, DPMM_EINVAL, "slot out of range");
    const size_t DP = (size_t)c->ma.DP;
    if (c->apairs_valid) {      // launched ahead with the posteriors?
        bool all = true;
        std::vector<int> rec((size_t)n);
        for (int i = 0; i < n && all; ++i) {
            const auto it = c->apairs_index.find(((uint32_t)slots_i[i] << 16) | (uint32_t)slots_j[i]);
            all = it != c->apairs_index.end() && !c->apairs_dirty[slots_i[i]] && !c->apairs_dirty[slots_j[i]];
            if (all) rec[i] = it->second;
        }
        if (all) {
            if (int rc = master_pinned(c, sizeof(double) * DPMM_MASTER_NSCALARS * (size_t)n)) return rc;
            HIPCHK(c, hipEventSynchronize(c->ev_pairs));
            double *sm = reinterpret_cast<double *>(c->h_master.get());      // (free: every user waits for its kernels before it returns)
            for (int i = 0; i < n; ++i) memcpy(sm + (size_t)i * DPMM_MASTER_NSCALARS, c->h_apairs + (size_t)rec[i] * DPMM_MASTER_NSCALARS, sizeof(double) * DPMM_MASTER_NSCALARS);
            *small = sm;
            return DPMM_OK;
        }
    }
    if (int rc = spec_join(c)) return rc;          // (a job launched ahead may still use the scratch matrices)
    if ((size_t)n > c->pair_cap) {
        HIPCHK(c, sync_stream(c, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream2));
        const size_t cap = grow_capacity((size_t)n, 64);
        c->pair_cap = 0;
        HIPCHK(c, c->d_pairs.alloc(sizeof(double) * cap * DP * DP));
        c->pair_cap = cap;
    }
    const size_t idx_bytes = (sizeof(int32_t) * 2 * (size_t)n + 63) & ~(size_t)63;
    if (int rc = master_pinned(c, idx_bytes + sizeof(double) * DPMM_MASTER_NSCALARS * (size_t)n)) return rc;
    HIPCHK(c, sync_stream(c, c->stream));
    int32_t *pr = reinterpret_cast<int32_t *>(c->h_master.get());
    for (int i = 0; i < n; ++i) { pr[2 * i] = slots_i[i]; pr[2 * i + 1] = slots_j[i]; }
    double *sm = reinterpret_cast<double *>(c->h_master + idx_bytes);
    HIPCHK(c, launch_niw_master_pairs(c->ma, pr, n, c->d_pairs, sm, c->stream));
    HIPCHK(c, sync_stream(c, c->stream));
    *small = sm;
    return DPMM_OK;
}

int dpmm_niw_master_put_rows(dpmm_ctx *c, const double *rows, int K) {
    if (!c || !rows) return DPMM_EINVAL;
    if (!c->master) return fail(c, DPMM_ESTATE, "dpmm_niw_master_setup first");
    if (int rc = check_K(c, K)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_capacity(c, K)) return rc;
    HIPCHK(c, sync_stream(c, c->stream));
    HIPCHK(c, hipMemcpy(c->d_out, rows, sizeof(double) * 2 * (size_t)K * (size_t)c->packed_stride, hipMemcpyHostToDevice));
    c->apairs_valid = false;
    if (K != c->K) c->have_params = false;
    c->K = K;
    return DPMM_OK;
}

int dpmm_niw_master_rows(dpmm_ctx *c, const int32_t *slots, int n, double *out) {
    if (!c || !slots || !out || n < 0) return DPMM_EINVAL;
    if (!c->master) return fail(c, DPMM_ESTATE, "dpmm_niw_master_setup first");
    if (n == 0) return DPMM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t stride = (size_t)c->packed_stride, bytes = sizeof(double) * 2 * (size_t)n * stride;
    for (int i = 0; i < n; ++i)
        if (slots[i] < 0 || slots[i] >= c->master_slots) return fail(c, DPMM_EINVAL, "slot out of range");
    // one gather kernel into pinned memory (n separate copies cost 6 us each), then a host copy to the caller's buffer
    if (int rc = ensure_out(c, bytes)) return rc;
    if (int rc = ensure_pinned(c, sizeof(int32_t) * (size_t)n + 64)) return rc;
    HIPCHK(c, sync_stream(c, c->stream));
    memcpy(c->h_pin, slots, sizeof(int32_t) * (size_t)n);
    HIPCHK(c, launch_niw_rows_gather(c->ma.rows_store, reinterpret_cast<const int32_t *>(c->h_pin.get()), n, (int64_t)stride,
                                     reinterpret_cast<double *>(c->h_out.get()), c->stream));
    HIPCHK(c, sync_stream(c, c->stream));
    memcpy(out, c->h_out, bytes);
    return DPMM_OK;
}

int dpmm_niw_master_draws(dpmm_ctx *c, int K, float *mu, float *R, float *logdet) {
    if (!c || !mu || !R || !logdet) return DPMM_EINVAL;
    if (!c->master || !c->draws_on_device || K != c->K) return fail(c, DPMM_ESTATE, "no device draws for this K");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_stream(c, c->stream));
    const size_t D = (size_t)c->D, DP = (size_t)c->ma.DP;
    std::vector<double> Y(3 * (size_t)K * DP * DP);
    std::vector<float> m(3 * (size_t)K * DP);
    HIPCHK(c, hipMemcpy(Y.data(), c->d_Y[c->draw_cur], sizeof(double) * Y.size(), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(m.data(), c->d_mu_draw[c->draw_cur], sizeof(float) * m.size(), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(logdet, c->d_ld_sigma[c->draw_cur], sizeof(float) * 3 * (size_t)K, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < 3 * (size_t)K; ++j) {
        for (size_t d = 0; d < D; ++d) mu[j * D + d] = m[j * DP + d];
        for (size_t r = 0; r < D; ++r)
            for (size_t cc = 0; cc < D; ++cc) R[(j * D + r) * D + cc] = cc >= r ? (float)Y[(j * DP + cc) * DP + r] : 0.f;
    }
    return DPMM_OK;
}

// ---- the Multinomial master's draws on the device ----------------------------------------------------------------------------
int dpmm_mult_master_setup(dpmm_ctx *c, const float *alpha, const float *alpha_outlier) {
    if (!c || !alpha) return DPMM_EINVAL;
    if (c->prior != DPMM_PRIOR_MULT) return fail(c, DPMM_EINVAL, "dpmm_mult_master_setup: the context is not Multinomial");
    if (c->D > DPMM_MULT_MASTER_MAXD) return fail(c, DPMM_ELIMIT, "D exceeds the device Dirichlet draw's limit");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_stream(c, c->stream));
    if (!c->d_malpha) HIPCHK(c, c->d_malpha.alloc(sizeof(float) * 2 * (size_t)c->ldx));
    HIPCHK(c, hipMemsetAsync(c->d_malpha, 0, sizeof(float) * 2 * (size_t)c->ldx, c->stream));
    HIPCHK(c, sync_stream(c, c->stream));
    HIPCHK(c, hipMemcpy(c->d_malpha, alpha, sizeof(float) * (size_t)c->D, hipMemcpyHostToDevice));
    if (alpha_outlier) HIPCHK(c, hipMemcpy(c->d_malpha + c->ldx, alpha_outlier, sizeof(float) * (size_t)c->D, hipMemcpyHostToDevice));
    c->mult_has_alpha1 = alpha_outlier != nullptr;
    for (int p = 0; p < 2; ++p) {
        const float *al = p ? alpha_outlier : alpha;
        double sa = 0.0, sl = 0.0;
        if (al) for (int d = 0; d < c->D; ++d) { sa += (double)al[d]; sl += lgamma((double)al[d]); }
        c->mult_prior_c[2 * p] = sa; c->mult_prior_c[2 * p + 1] = sl;
    }
    if (!c->d_mpairs) HIPCHK(c, c->d_mpairs.alloc(sizeof(int32_t) * 2 * DPMM_MULT_MASTER_MAXPAIRS));
    if (!c->h_marg) HIPCHK(c, c->h_marg.alloc(sizeof(double) * (6 * DPMM_MAX_CLUSTERS + DPMM_MULT_MASTER_MAXPAIRS)));
    c->marg_valid = false; c->marg_req = false; c->mpairs_shadow.clear();
    if (!c->h_draw) HIPCHK(c, c->h_draw.alloc(sizeof(float) * 3 * DPMM_MAX_CLUSTERS));
    c->mult_master = true;
    return DPMM_OK;
}

int dpmm_mult_master_put_rows(dpmm_ctx *c, const double *rows, int K) {
    if (!c || !rows) return DPMM_EINVAL;
    if (!c->mult_master) return fail(c, DPMM_ESTATE, "dpmm_mult_master_setup first");
    if (int rc = check_K(c, K)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_capacity(c, K)) return rc;
    HIPCHK(c, sync_stream(c, c->stream));
    HIPCHK(c, hipMemcpy(c->d_out, rows, sizeof(double) * 2 * (size_t)K * (size_t)c->packed_stride, hipMemcpyHostToDevice));
    c->K = K;
    c->rows_full_K = K;
    c->marg_valid = false;
    c->mspec_valid = false;
    c->cache_force = true;            // (the rows did not come from this context's labels: nothing to derive from)
    return DPMM_OK;
}

int dpmm_mult_master_draw(dpmm_ctx *c, uint32_t epoch, int K, int outlier_first, const float *lr, const float *w) {
    if (!c || !lr || !w) return DPMM_EINVAL;
    if (!c->mult_master) return fail(c, DPMM_ESTATE, "dpmm_mult_master_setup first");
    if (int rc = check_K(c, K)) return rc;
    if (c->rows_full_K != K) return fail(c, DPMM_ESTATE, "dpmm_mult_master_draw: the last statistics pass did not leave the rows of all K clusters");
    if (outlier_first && !c->mult_has_alpha1) return fail(c, DPMM_ESTATE, "dpmm_mult_master_draw: no outlier prior was set up");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_capacity(c, K)) return rc;
    // cst[3k] = log w_k, cst[3k+1+s] = log lr[k][s] through the pinned block.  The block is re-used once the copy of the PREVIOUS call has read
    // it -- known from the host's waits since, not by waiting for the stream here: the stream may be carrying the draws launched ahead and the late
    // rows, and waiting for those would put them back on the host's path
    if (c->cst_inflight && c->cst_gen == c->sync_gen) HIPCHK(c, sync_stream(c, c->stream));     // (never in the engine's loop: dpmm_step_stats waited in between)
    float *hcst = reinterpret_cast<float *>(c->h_draw.get());
    for (int k = 0; k < K; ++k) { hcst[3 * k] = logf(w[k]); hcst[3 * k + 1] = logf(lr[2 * k]); hcst[3 * k + 2] = logf(lr[2 * k + 1]); }
    HIPCHK(c, launch_copy_bytes(c->d_cst, hcst, sizeof(float) * 3 * K, c->stream));
    c->cst_inflight = true; c->cst_gen = c->sync_gen;
    if (c->mspec_valid && c->mspec_epoch == epoch && c->mspec_K == K && c->mspec_outlier == (outlier_first ? 1 : 0)) {
        // made behind the statistics pass (dpmm_step_stats) from these very rows: the two sets of buffers change places
        std::swap(c->d_raw, c->d_raw2); std::swap(c->d_Rp, c->d_Rp2); std::swap(c->d_Lp16, c->d_Lp16_2); std::swap(c->rp_current, c->rp2_current);
        c->mspec_used += 1;
    } else {
        HIPCHK(c, launch_mult_dirichlet(c->d_out, c->packed_stride, c->d_malpha, c->mult_has_alpha1 ? c->d_malpha + c->ldx : nullptr, outlier_first, c->D, c->ldx,
                                        K, c->seed, epoch, c->d_raw, c->stream));
        c->rp_current = !(c->x_u8 || c->x_bf16_exact || c->x_sparse);
        if (c->rp_current) HIPCHK(c, launch_mult_pack(c->d_raw, c->d_Rp, 3 * K, c->ldx, c->stream));
        if (c->x_sparse) if (int rc = pack_sparse_image(c, c->d_raw, c->d_Rp, K)) return rc;
        if (c->x_u8) HIPCHK(c, launch_mult_pack_u8(c->d_raw, c->d_Lp16, 3 * K, c->ldx, c->ld8, c->stream));
        else if (c->x_bf16_exact) HIPCHK(c, launch_mult_pack_bf16(c->d_raw, c->d_Lp16, 3 * K, c->ldx, c->stream));
    }
    c->mspec_valid = false;
    c->mdraw_epoch = epoch; c->mdraw_seen = true;
    c->K = K;
    c->have_params = true;
    c->predictive = false;
    c->draws_on_device = true;
    return DPMM_OK;
}

int dpmm_mult_master_rows_on_demand(dpmm_ctx *c, int on) {
    if (!c) return DPMM_EINVAL;
    if (!c->mult_master) return fail(c, DPMM_ESTATE, "dpmm_mult_master_setup first");
    c->rows_on_demand = on != 0;
    return DPMM_OK;
}

int dpmm_mult_master_rows_wait(dpmm_ctx *c) {
    if (!c) return DPMM_EINVAL;
    if (c->rows_late) {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, sync_stream(c, c->stream));
        c->rows_late = false;
    }
    return DPMM_OK;
}

int dpmm_debug_mult_draws_ahead(dpmm_ctx *c, long long *used) {
    if (!c || !used) return DPMM_EINVAL;
    *used = c->mspec_used;
    return DPMM_OK;
}

int dpmm_mult_master_draws(dpmm_ctx *c, int K, float *logp) {
    if (!c || !logp) return DPMM_EINVAL;
    if (!c->mult_master || !c->draws_on_device || K != c->K) return fail(c, DPMM_ESTATE, "no device draws for this K");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_stream(c, c->stream));
    HIPCHK(c, hipMemcpy2D(logp, sizeof(float) * (size_t)c->D, c->d_raw, sizeof(float) * (size_t)c->ldx, sizeof(float) * (size_t)c->D, 3 * (size_t)K,
                          hipMemcpyDeviceToHost));
    return DPMM_OK;
}

// the log-marginal kernel over the rows of the last full pass + the pairs asked for (asynchronous; results in the pinned block)
static int mult_marginals_launch(dpmm_ctx *c) {
    c->marg_req = false;
    c->marg_behind_ev = false;
    const int K = c->K;
    if (!c->mult_master || c->rows_full_K != K) return DPMM_OK;           // (nothing to answer from: dpmm_mult_master_marginals will say so)
    if (c->marg_req_outlier && !c->mult_has_alpha1) return DPMM_OK;
    int np = (int)(c->mpairs_req.size() / 2);
    for (int32_t k : c->mpairs_req) if (k < 0 || k >= K) { np = 0; break; }
    if (np > 0) if (int rc = device_list(c, c->d_mpairs, c->mpairs_shadow, c->mpairs_req.data(), 2 * (size_t)np)) return rc;
    HIPCHK(c, launch_mult_marginals(c->d_out, c->packed_stride, c->d_malpha, c->mult_has_alpha1 ? c->d_malpha + c->ldx : nullptr, c->marg_req_outlier,
                                    c->D, K, c->d_mpairs, np, c->mult_prior_c, c->h_marg, c->stream));
    c->marg_valid = true; c->marg_K = K; c->marg_np = np;
    return DPMM_OK;
}

int dpmm_mult_master_pairs_ahead(dpmm_ctx *c, int outlier_first, const int32_t *ki, const int32_t *kj, int n) {
    if (!c || n < 0 || (n > 0 && (!ki || !kj))) return DPMM_EINVAL;
    if (!c->mult_master) return fail(c, DPMM_ESTATE, "dpmm_mult_master_setup first");
    c->mpairs_req.clear();
    if (n <= DPMM_MULT_MASTER_MAXPAIRS)
        for (int p = 0; p < n; ++p) { c->mpairs_req.push_back(ki[p]); c->mpairs_req.push_back(kj[p]); }
    c->marg_req = true; c->marg_req_outlier = outlier_first ? 1 : 0;
    return DPMM_OK;
}

int dpmm_mult_master_marginals(dpmm_ctx *c, int K, const double **rows_nl, const double **pairs_l, int *npairs) {
    if (!c || !rows_nl || !pairs_l || !npairs) return DPMM_EINVAL;
    if (!c->mult_master) return fail(c, DPMM_ESTATE, "dpmm_mult_master_setup first");
    if (int rc = check_K(c, K)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (!(c->marg_valid && c->marg_K == K && c->rows_full_K == K)) {
        if (c->rows_full_K != K || K != c->K) return fail(c, DPMM_ESTATE, "dpmm_mult_master_marginals: the last statistics pass did not leave the rows of all K clusters");
        c->marg_valid = false;
        if (int rc = mult_marginals_launch(c)) return rc;
        if (!c->marg_valid) return fail(c, DPMM_ESTATE, "dpmm_mult_master_marginals: no outlier prior was set up");
    }
    if (c->marg_behind_ev) HIPCHK(c, sync_event(c, c->ev_rows));      // (dpmm_step_stats waited for it already; the stream still carries the draws launched ahead)
    else HIPCHK(c, sync_stream(c, c->stream));        // (no-op behind dpmm_step_stats, which waited for the kernel with the rows)
    *rows_nl = c->h_marg; *pairs_l = c->h_marg + 6 * (size_t)K; *npairs = c->marg_np;
    return DPMM_OK;
}

int dpmm_debug_niw_draw_inputs(dpmm_ctx *c, uint32_t epoch, int K, const int32_t *slot_of_cluster, double *A, double *xi) {
    if (!c || !slot_of_cluster || !A || !xi) return DPMM_EINVAL;
    if (!c->master) return fail(c, DPMM_ESTATE, "dpmm_niw_master_setup first");
    if (K < 1 || K > DPMM_MAX_CLUSTERS) return fail(c, DPMM_EINVAL, "bad K");
    HIPCHK(c, hipSetDevice(c->device));
    for (int k = 0; k < K; ++k)
        if (slot_of_cluster[k] < 0 || slot_of_cluster[k] >= c->master_slots) return fail(c, DPMM_EINVAL, "slot without a posterior on the device");
    const size_t D = (size_t)c->D, nA = 3 * (size_t)K * D * D, nx = 3 * (size_t)K * D;
    DevBuf<double> dA, dxi;
    DevBuf<int32_t> dsl;
    HIPCHK(c, sync_stream(c, c->stream));
    hipError_t e = dA.alloc(sizeof(double) * nA);
    if (e == hipSuccess) e = dxi.alloc(sizeof(double) * nx);
    if (e == hipSuccess) e = dsl.alloc(sizeof(int32_t) * K);
    if (e == hipSuccess) e = hipMemsetAsync(dA, 0, sizeof(double) * nA, c->stream);
    if (e == hipSuccess) e = hipMemcpy(dsl, slot_of_cluster, sizeof(int32_t) * K, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_niw_draw_inputs(c->ma, dsl, K, epoch, dA, dxi, c->stream);
    if (e == hipSuccess) e = sync_stream(c, c->stream);
    if (e == hipSuccess) e = hipMemcpy(A, dA, sizeof(double) * nA, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(xi, dxi, sizeof(double) * nx, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { c->err = std::string("dpmm_debug_niw_draw_inputs: ") + hipGetErrorString(e); return DPMM_EHIP; }
    return DPMM_OK;
}

int dpmm_suffstats_packed(dpmm_ctx *c, const int64_t *idx, int n_idx, double *out) {
    if (!c || !out) return DPMM_EINVAL;
    const double *pk = nullptr;
    if (int rc = dpmm_suffstats_host(c, idx, n_idx, &pk)) return rc;
    memcpy(out, pk, sizeof(double) * 2 * c->K * (size_t)c->packed_stride);
    return DPMM_OK;
}

int dpmm_unpack_suffstats(const dpmm_ctx *c, int K, const double *packed, double *N, double *sum, double *S) {
    if (!c || !packed || !N || !sum) return DPMM_EINVAL;
    const int D = c->D;
    const int64_t ps = c->packed_stride;
    for (int k = 0; k < K; ++k) {
        const double *l = packed + (size_t)(2 * k) * ps, *r = packed + (size_t)(2 * k + 1) * ps;
        N[3 * k + 1] = l[0]; N[3 * k + 2] = r[0]; N[3 * k] = l[0] + r[0];
        for (int d = 0; d < D; ++d) {
            sum[(size_t)(3 * k + 1) * D + d] = l[1 + d];
            sum[(size_t)(3 * k + 2) * D + d] = r[1 + d];
            sum[(size_t)(3 * k) * D + d] = l[1 + d] + r[1 + d];
        }
        if (S && c->prior == DPMM_PRIOR_NIW) {
            double *Sc = S + (size_t)(3 * k) * D * D, *Sl = Sc + (size_t)D * D, *Sr = Sl + (size_t)D * D;
            for (int a = 0; a < D; ++a)
                for (int b = 0; b <= a; ++b) {
                    const double vl = l[1 + D + (size_t)a * (a + 1) / 2 + b], vr = r[1 + D + (size_t)a * (a + 1) / 2 + b];
                    Sl[(size_t)a * D + b] = Sl[(size_t)b * D + a] = vl;
                    Sr[(size_t)a * D + b] = Sr[(size_t)b * D + a] = vr;
                    Sc[(size_t)a * D + b] = Sc[(size_t)b * D + a] = vl + vr;
                }
        }
    }
    return DPMM_OK;
}

static int upload_idx(dpmm_ctx *c, const int64_t *a, const int64_t *b, int n, int limit) {
    if (n < 0 || n > 2 * DPMM_MAX_CLUSTERS) return fail(c, DPMM_ELIMIT, "index list too long");
    std::vector<int32_t> h((size_t)(b ? 2 : 1) * n);
    for (int j = 0; j < n; ++j) {
        if (a[j] < 1 || a[j] > limit) return fail(c, DPMM_EINVAL, "cluster index out of range");
        h[j] = (int32_t)(a[j] - 1);
        if (b) {
            if (b[j] < 1 || b[j] > limit) return fail(c, DPMM_EINVAL, "cluster index out of range");
            h[n + j] = (int32_t)(b[j] - 1);
        }
    }
    if (int rc = ensure_pinned(c, sizeof(int32_t) * h.size())) return rc;
    HIPCHK(c, sync_stream(c, c->stream));
    memcpy(c->h_pin, h.data(), sizeof(int32_t) * h.size());
    HIPCHK(c, launch_copy_bytes(c->d_small, c->h_pin, sizeof(int32_t) * h.size(), c->stream));
    return DPMM_OK;
}

int dpmm_split(dpmm_ctx *c, const int64_t *idx, const int64_t *new_idx, int n, uint32_t epoch) {
    if (!c) return DPMM_EINVAL;
    if (!c->have_labels) return fail(c, DPMM_ESTATE, "labels not initialised");
    if (n == 0) return DPMM_OK;
    if (!idx || !new_idx) return fail(c, DPMM_EINVAL, "null index list");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = upload_idx(c, idx, new_idx, n, DPMM_MAX_CLUSTERS)) return rc;
    if (c->n > 0) HIPCHK(c, launch_split(c->dbins, c->n, c->first, c->d_small, n, c->seed, epoch, c->stream));
    c->rows_full_K = -1;              // (the rows of the last pass no longer describe these labels)
    return DPMM_OK;
}

int dpmm_merge(dpmm_ctx *c, const int64_t *idx, const int64_t *new_idx, int n) {
    if (!c) return DPMM_EINVAL;
    if (!c->have_labels) return fail(c, DPMM_ESTATE, "labels not initialised");
    if (n == 0) return DPMM_OK;
    if (!idx || !new_idx) return fail(c, DPMM_EINVAL, "null index list");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = upload_idx(c, idx, new_idx, n, DPMM_MAX_CLUSTERS)) return rc;
    if (c->n > 0) HIPCHK(c, launch_merge(c->dbins, c->n, c->d_small, n, c->stream));
    c->rows_full_K = -1;
    return DPMM_OK;
}

int dpmm_remove_empty(dpmm_ctx *c, const int64_t *pts_count, int K) {
    if (!c) return DPMM_EINVAL;
    if (!c->have_labels) return fail(c, DPMM_ESTATE, "labels not initialised");
    if (!pts_count || K < 1 || K > DPMM_MAX_CLUSTERS) return fail(c, DPMM_EINVAL, "bad pts_count / K");
    HIPCHK(c, hipSetDevice(c->device));
    // literal simulation of remove_empty_clusters_worker! on the identity label vector -> lookup table
    std::vector<int32_t> map(DPMM_MAX_CLUSTERS);
    for (int l = 1; l <= DPMM_MAX_CLUSTERS; ++l) {
        int v = l, removed = 0;
        for (int k = 1; k <= K; ++k)
            if (pts_count[k - 1] == 0) {
                if (v > k - removed) v -= 1;
                removed += 1;
            }
        map[l - 1] = v - 1;
    }
    if (int rc = ensure_pinned(c, sizeof(int32_t) * map.size())) return rc;
    HIPCHK(c, sync_stream(c, c->stream));
    memcpy(c->h_pin, map.data(), sizeof(int32_t) * map.size());
    HIPCHK(c, launch_copy_bytes(c->d_small, c->h_pin, sizeof(int32_t) * map.size(), c->stream));
    if (c->n > 0) HIPCHK(c, launch_remap(c->dbins, c->n, c->d_small, c->stream));
    c->rows_full_K = -1;
    return DPMM_OK;
}

int dpmm_reset_sublabels(dpmm_ctx *c, const int64_t *idx, int n, uint32_t epoch) {
    if (!c) return DPMM_EINVAL;
    if (!c->have_labels) return fail(c, DPMM_ESTATE, "labels not initialised");
    HIPCHK(c, hipSetDevice(c->device));
    if (idx) {
        if (n == 0) return DPMM_OK;
        if (int rc = upload_idx(c, idx, nullptr, n, DPMM_MAX_CLUSTERS)) return rc;
    }
    if (c->n > 0) HIPCHK(c, launch_reset_sub(c->dbins, c->n, c->first, idx ? c->d_small : nullptr, idx ? n : 0, c->seed, epoch, c->stream));
    c->rows_full_K = -1;
    return DPMM_OK;
}

static int smart_buffers(dpmm_ctx *c) {
    if (c->d_proj) return DPMM_OK;
    const size_t n = (size_t)std::max<int64_t>(c->n, 1);
    HIPCHK(c, c->d_proj.alloc(sizeof(double) * n));
    HIPCHK(c, c->d_vals.alloc(sizeof(double) * n));
    HIPCHK(c, c->d_smart.alloc(sizeof(double) * (4 * (size_t)smart_groups() + 8 + 2 * (size_t)c->D)));
    return DPMM_OK;
}
static int smart_check(dpmm_ctx *c, int64_t cluster) {
    if (!c->have_points || !c->have_labels) return fail(c, DPMM_ESTATE, "smart split needs points and labels");
    if (cluster < 1 || cluster > DPMM_MAX_CLUSTERS) return fail(c, DPMM_EINVAL, "cluster index out of range");
    return DPMM_OK;
}

int dpmm_smart_project(dpmm_ctx *c, int64_t cluster, const double *v, const double *mu, double *values, int64_t *count) {
    if (!c || !v || !mu || !count) return DPMM_EINVAL;
    if (int rc = smart_check(c, cluster)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = smart_buffers(c)) return rc;
    *count = 0;
    if (c->n == 0) return DPMM_OK;
    double *d_v = c->d_smart + 4 * (size_t)smart_groups() + 8, *d_mu = d_v + c->D;
    unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(c->d_smart + 4 * (size_t)smart_groups() + 4);
    HIPCHK(c, hipMemcpyAsync(d_v, v, sizeof(double) * c->D, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_mu, mu, sizeof(double) * c->D, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), c->stream));
    HIPCHK(c, launch_smart_project(c->dbins, c->dX, c->ldx, c->n, c->D, (int)(cluster - 1), d_v, d_mu, c->d_proj, c->d_vals, d_cnt, c->stream));
    unsigned long long h = 0;
    HIPCHK(c, hipMemcpyAsync(&h, d_cnt, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, sync_stream(c, c->stream));
    *count = (int64_t)h;
    if (values && h > 0) HIPCHK(c, hipMemcpy(values, c->d_vals, sizeof(double) * h, hipMemcpyDeviceToHost));
    return DPMM_OK;
}

int dpmm_smart_kmeans_iter(dpmm_ctx *c, int64_t cluster, double m_lo, double m_hi, double *out4) {
    if (!c || !out4) return DPMM_EINVAL;
    if (int rc = smart_check(c, cluster)) return rc;
    if (!c->d_proj) return fail(c, DPMM_ESTATE, "dpmm_smart_project has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    out4[0] = out4[1] = out4[2] = out4[3] = 0.;
    if (c->n == 0) return DPMM_OK;
    double *d_out = c->d_smart + 4 * (size_t)smart_groups();
    HIPCHK(c, launch_smart_kmeans(c->dbins, c->d_proj, c->n, (int)(cluster - 1), m_lo, m_hi, c->d_smart, d_out, c->stream));
    HIPCHK(c, hipMemcpyAsync(out4, d_out, sizeof(double) * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, sync_stream(c, c->stream));
    return DPMM_OK;
}

int dpmm_smart_assign(dpmm_ctx *c, int64_t cluster, double m_lo, double m_hi) {
    if (!c) return DPMM_EINVAL;
    if (int rc = smart_check(c, cluster)) return rc;
    if (!c->d_proj) return fail(c, DPMM_ESTATE, "dpmm_smart_project has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n > 0) HIPCHK(c, launch_smart_assign(c->dbins, c->d_proj, c->n, (int)(cluster - 1), m_lo, m_hi, c->stream));
    return DPMM_OK;
}

int dpmm_set_ground_truth(dpmm_ctx *c, const int64_t *gt, int n_gt) {
    if (!c) return DPMM_EINVAL;
    if ((!gt && c->n > 0) || n_gt < 1 || n_gt > 65536) return fail(c, DPMM_EINVAL, "bad ground truth");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_gt) HIPCHK(c, c->d_gt.alloc(sizeof(int32_t) * (size_t)std::max<int64_t>(c->n, 1)));
    HIPCHK(c, c->d_cont.alloc(sizeof(unsigned long long) * (size_t)DPMM_MAX_CLUSTERS * n_gt));
    if (c->n > 0) {
        DevBuf<int64_t> tmp;
        HIPCHK(c, tmp.alloc(sizeof(int64_t) * (size_t)c->n));
        hipError_t e = hipMemcpyAsync(tmp, gt, sizeof(int64_t) * c->n, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = launch_i64_to_i32(c->d_gt, tmp, c->n, c->stream);
        if (e == hipSuccess) e = sync_stream(c, c->stream);
        if (e != hipSuccess) { c->err = std::string("dpmm_set_ground_truth: ") + hipGetErrorString(e); return DPMM_EHIP; }
    }
    c->n_gt = n_gt;
    return DPMM_OK;
}

int dpmm_contingency(dpmm_ctx *c, int K, int64_t *counts) {
    if (!c || !counts) return DPMM_EINVAL;
    if (!c->d_gt || !c->have_labels) return fail(c, DPMM_ESTATE, "contingency needs labels and dpmm_set_ground_truth");
    if (int rc = check_K(c, K)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = sizeof(unsigned long long) * (size_t)K * c->n_gt;
    if (int rc = ensure_pinned(c, bytes)) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_cont, 0, bytes, c->stream));
    if (c->n > 0) HIPCHK(c, launch_contingency(c->dbins, c->d_gt, c->n, K, c->n_gt, c->d_cont, c->stream));
    HIPCHK(c, launch_copy_bytes(c->h_pin, c->d_cont, bytes, c->stream));
    HIPCHK(c, sync_stream(c, c->stream));
    memcpy(counts, c->h_pin, bytes);
    return DPMM_OK;
}

int dpmm_sync(dpmm_ctx *c) {
    if (!c) return DPMM_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_stream(c, c->stream));
    return DPMM_OK;
}

#ifdef DPMM_STAMPS
// diagnostic builds only: copy the per-wave phase cycle sums of the last NIW sweep
int dpmm_dev_stamps(dpmm_ctx *c, unsigned long long *out, int nwaves) {
    hipStreamSynchronize(c->stream);
    hipMemcpy(out, g_dbg, sizeof(unsigned long long) * 16 * nwaves, hipMemcpyDeviceToHost);
    return c->sweep_grid * 4;
}
#endif

void *dpmm_stream(dpmm_ctx *c) { return c ? (void *)c->stream : nullptr; }

int dpmm_set_option(dpmm_ctx *c, int option, double value) {
    if (!c) return DPMM_EINVAL;
    switch (option) {
        case DPMM_OPT_SCREEN_MARGIN: if (!(value >= 0)) return fail(c, DPMM_EINVAL, "margin < 0"); c->opt_margin = (float)value; return DPMM_OK;
        case DPMM_OPT_TAIL_SCREEN: c->opt_tail = value != 0; return DPMM_OK;
        case DPMM_OPT_PRESCREEN: c->opt_prescreen = value < 0 ? -1 : (value != 0); return DPMM_OK;
        case DPMM_OPT_ORDERED_SWEEP: c->opt_ordered = value != 0; return DPMM_OK;
        case DPMM_OPT_MULT_FORCE_F32:
            if (c->have_points) return fail(c, DPMM_ESTATE, "DPMM_OPT_MULT_FORCE_F32 must be set before the points are uploaded");
            c->opt_force_f32 = value != 0; return DPMM_OK;
        case DPMM_OPT_STATS_ITEMS:
            if (c->Kcap > 0) return fail(c, DPMM_ESTATE, "DPMM_OPT_STATS_ITEMS must be set before the first parameters / K");
            if (value >= 1) c->chunk_dense = c->chunk = (int)std::max<int64_t>((c->prior == DPMM_PRIOR_NIW && c->D <= 64) ? 32 : 256, ((c->n + (int64_t)value - 1) / (int64_t)value + 3) / 4 * 4);
            if (c->x_sparse) return set_points_chunk(c, true);
            return DPMM_OK;
        case DPMM_OPT_STATS_GROUPS: c->opt_stats_groups = value > 0 ? (int)value : 0; return DPMM_OK;
        case DPMM_OPT_TRACE_SLOW: c->opt_trace = value != 0; return DPMM_OK;
        case DPMM_OPT_LOGLIK_REF_CONST: c->opt_ref_const = value != 0; return DPMM_OK;
        case DPMM_OPT_WAVE_PRIO: c->opt_prio = value != 0; return DPMM_OK;
        case DPMM_OPT_MULT_DRAWS_AHEAD: c->opt_mult_draws_ahead = value != 0; c->mspec_valid = false; return DPMM_OK;
        case DPMM_OPT_SWEEP_QUEUE_ROUNDS: c->opt_queue_rounds = value < 0 ? -1 : (int)value; return DPMM_OK;
        case DPMM_OPT_BALL_SCREEN: c->opt_ball = value != 0; return DPMM_OK;
        case DPMM_OPT_STATS_DERIVE: c->opt_derive = value != 0; c->cache_force = true; return DPMM_OK;
        case DPMM_OPT_NOISE_AHEAD: c->opt_noise_ahead = value < 0 ? -1 : (value != 0); return DPMM_OK;
        case DPMM_OPT_REF_BRACKET: c->opt_bracket = value != 0; return DPMM_OK;
        case DPMM_OPT_COMM_TIMEOUT_MS: c->comm_timeout_ms = value > 0 ? (int)std::min(value, 2.0e9) : 0; return DPMM_OK;
        case DPMM_OPT_BF16_SCREENS: c->opt_bf16scr = value != 0; return DPMM_OK;
        case DPMM_OPT_MASTER_POLL: c->opt_master_poll = value != 0; return DPMM_OK;
        case DPMM_OPT_PAIR_BALL: c->opt_pair_ball = value != 0; if (!c->opt_pair_ball) c->have_pb = false; return DPMM_OK;      // (ON takes effect with the next parameter set)
        case DPMM_OPT_LEAN_NORM_CERT: c->opt_lean_norm_cert = (value == 2 || value == 3) ? value : (value != 0); c->cert_cool = 0; c->cert_fb = false; return DPMM_OK;      // (the table's sn2 block follows with the next parameter set)
        case DPMM_OPT_LEAN_DIRECTION: c->opt_lean_dir = value != 0; c->lean_off = 0; c->lean_backoff = 15; c->lean_ran = false; return DPMM_OK;
        case DPMM_OPT_CHAIN_FUSION: c->opt_chain = value < 0 ? (0x7fffffff & ~(8 | 32)) : (int)value; return DPMM_OK;
        case DPMM_OPT_LEAN_TILES: c->opt_lean = value != 0; c->lean_off = 0; c->lean_backoff = 15; c->lean_ran = false; return DPMM_OK;
        case DPMM_OPT_B3_SUBLABELS: c->opt_b3 = value != 0; if (!c->opt_b3) c->have_b3 = false; return DPMM_OK;      // (switching it ON takes effect with the next parameter set: its images are packed behind the parameters)
        case DPMM_OPT_DIRECTION_SCREEN:
            c->opt_direction = value < 0 ? -1 : (value != 0);
            if (c->opt_direction == 0) { c->sp_ready = false; c->sp_regime = false; }
            return DPMM_OK;
        case DPMM_OPT_ONE_COLLECTIVE: c->opt_one_collective = value < 0 ? -1 : (value != 0); return DPMM_OK;
        case DPMM_OPT_SORT_TILE: {
            const int t = (int)value;
            if (t != SORT_TILE && t != SORT_TILE_SMALL) return fail(c, DPMM_EINVAL, "DPMM_OPT_SORT_TILE: 512 or 2048");
            if (t < c->sort_tile_min) {          // tables for the smaller tile: allocated when asked for (behind everything that still reads the old ones)
                if (c->n > 16000000) return fail(c, DPMM_ELIMIT, "DPMM_OPT_SORT_TILE: 512-point tiles are limited to shards of 16e6 points");
                HIPCHK(c, hipSetDevice(c->device));
                HIPCHK(c, sync_stream(c, c->stream));
                const int nt = (int)((c->n + t - 1) / t);
                const size_t nbmax = 2 * DPMM_MAX_CLUSTERS;
                DevBuf<int32_t> th, tc, tsp;      // all three, then the old ones go
                if (th.alloc(sizeof(int32_t) * nbmax * (size_t)std::max(1, nt)) != hipSuccess || tc.alloc(sizeof(int32_t) * nbmax * (size_t)std::max(1, nt)) != hipSuccess ||
                    tsp.alloc(sizeof(int32_t) * (size_t)STEP_SPEC_MAX_BINS * (size_t)std::max(1, nt)) != hipSuccess)
                    return fail(c, DPMM_EHIP, "DPMM_OPT_SORT_TILE: out of device memory for the 512-point tile tables");
                c->sort_mem.tile_hist = std::move(th); c->sort_mem.tile_cnt = std::move(tc); c->sort_mem.tile_spec = std::move(tsp);
                sort_view(c);
                c->nt_sort = nt; c->sort_tile_min = t;
            }
            c->sb.tile = t; return DPMM_OK;          // (the tile tables are rebuilt by every pass; perm stays a valid order)
        }
        case DPMM_OPT_KERNEL_TIMING:
            c->opt_timing = (int)value & 15;
            if (!(c->opt_timing & 1)) c->have_sweep_ev = false;
            if (!(c->opt_timing & 2)) c->have_stats_ev = false;
            if (!(c->opt_timing & 4)) c->have_comm_ev[0] = c->have_comm_ev[1] = false;
            return DPMM_OK;
        case DPMM_OPT_SWEEP_GRID:
            if (value > 0) c->sweep_grid = (int)std::min<double>(std::min<double>(value, (double)c->sweep_grid_max), (double)std::max<int64_t>(1, c->ntiles));   // scratch is sized for the default
            return DPMM_OK;
        case DPMM_OPT_MULT_NO_U8:
            if (c->have_points) return fail(c, DPMM_ESTATE, "DPMM_OPT_MULT_NO_U8 must be set before the points are uploaded");
            c->opt_no_u8 = value != 0; return DPMM_OK;
        case DPMM_OPT_SCORE_TABLE_MB: c->opt_score_mb = (value < 0 || value != value) ? 128.0 : value; return DPMM_OK;
        case DPMM_OPT_SCORE_MISSING:
            if (value != 0 && c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, "DPMM_OPT_SCORE_MISSING: the Multinomial prior has no missing features");
            c->opt_score_missing = value != 0; return DPMM_OK;
        case DPMM_OPT_TYPICALITY_GAPS:
            if (value != 0 && c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, "DPMM_OPT_TYPICALITY_GAPS: the Multinomial prior has no missing features");
            c->opt_typ_gaps = value != 0; return DPMM_OK;
        default: return fail(c, DPMM_EINVAL, "unknown option");
    }
}

int dpmm_last_sweep_work(dpmm_ctx *c, uint64_t *out16) {
    if (!c || !out16) return DPMM_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_stream(c, c->stream));
    std::vector<unsigned long long> h((size_t)DPMM_WORK_PER_WAVE * (size_t)c->work_waves);
    if (!h.empty()) HIPCHK(c, hipMemcpy(h.data(), c->d_work + DPMM_WORK_SLOTS, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < 16; ++i) out16[i] = 0;
    unsigned long long w7_lo = 0, w7_hi = 0, w6_lo = 0, w6_hi = 0;
    for (size_t w = 0; w < (size_t)c->work_waves; ++w) {
        for (int i = 0; i < 4; ++i) out16[i] += h[DPMM_WORK_PER_WAVE * w + i];
        out16[8] += h[DPMM_WORK_PER_WAVE * w + 4];
        out16[11] += h[DPMM_WORK_PER_WAVE * w + 5];
        w6_lo += h[DPMM_WORK_PER_WAVE * w + 6] & 0xFFFFFFFFull; w6_hi += h[DPMM_WORK_PER_WAVE * w + 6] >> 32;      // (bf16 top screens | tiles settled by the norm certificate)
        // slot 7 packs two counters per wave -- low half: direction screens (8 bf16 matrix instructions per 16 clusters + 4 Float32 row sums
        // each); high half: bf16 three-plane sub-cluster evaluations (niw_lean.hip).  The halves are summed SEPARATELY over the waves (a raw
        // 64-bit sum lets the low halves' carry run into the evaluation count after a few thousand launches between two reads: ADVICE r5)
        w7_lo += h[DPMM_WORK_PER_WAVE * w + 7] & 0xFFFFFFFFull; w7_hi += h[DPMM_WORK_PER_WAVE * w + 7] >> 32;
    }
    out16[13] = std::min<unsigned long long>(w6_lo, 0xFFFFFFFFull) | (std::min<unsigned long long>(w6_hi, 0xFFFFFFFFull) << 32);
    out16[15] = std::min<unsigned long long>(w7_lo, 0xFFFFFFFFull) | (std::min<unsigned long long>(w7_hi, 0xFFFFFFFFull) << 32);      // (each half saturates at 2^32 - 1)
    // totals of the launches since the previous call (out16[7] of them); the slots start again from zero
    const long long launches = c->work_launches;
    if (!h.empty()) HIPCHK(c, hipMemsetAsync(c->d_work + DPMM_WORK_SLOTS, 0, sizeof(unsigned long long) * h.size(), c->stream));
    c->work_launches = 0; c->work_waves = 0;
    // matrix instructions per unit of work, per WAVE (v_mfma_f32_16x16x4_f32, 2048 flops each)
    int mf_full = 0, mf_scr = 0;
    if (c->prior == DPMM_PRIOR_NIW) {
        const int NB = c->NB, NP = NB * (NB + 1) / 2;
        const int NG = NB <= 4 ? 4 : 2;                       // points per wave / 16 (launch_niw_sweep configurations)
        mf_full = NP * 4 * NG + (NB <= 4 ? NG : 0);           // block pairs x 4 k-steps x NG (+ the ones-MFMA row sums of the direct kernel)
        mf_scr = 4 * NG;                                       // the 16-row screen: one block, 4 k-steps, NG point groups
    }
    out16[4] = (uint64_t)mf_full; out16[5] = (uint64_t)mf_scr; out16[6] = 2048; out16[7] = (uint64_t)launches;
    out16[9] = c->NB == 16 ? 288 : (c->NB == 8 ? 80 : 48); out16[10] = 16384;      // bf16 matrix instructions of a reference bracket per wave tile
    out16[12] = 8; out16[14] = 16;                           // bf16 matrix instructions of a bottom / top screen (+ 4 Float32 row sums per top screen)                          // a reference bracket: 6 fragments x 2 passes x 4 point groups of v_mfma_f32_16x16x32_bf16 (2 * 16 * 16 * 32 flops each)
    return DPMM_OK;
}

// ---- the collective ------------------------------------------------------------------------------------------------------
int dpmm_comm_use_library(const char *path) {
    g_rccl_path = path ? path : "";
    return DPMM_OK;
}

int dpmm_comm_unique_id(void *out128) {
    if (!out128) return DPMM_EINVAL;
    Rccl &r = rccl();
    if (!r.handle || !r.err.empty()) return fail(nullptr, DPMM_ECOMM, r.err.empty() ? "RCCL unavailable" : r.err);
    const int rc = r.GetUniqueId(out128);
    if (rc != 0) return fail(nullptr, DPMM_ECOMM, std::string("ncclGetUniqueId: ") + r.GetErrorString(rc));
    return DPMM_OK;
}

int dpmm_comm_init(dpmm_ctx *c, const void *unique_id128, int rank, int world) {
    if (!c || !unique_id128) return DPMM_EINVAL;
    if (world < 1 || rank < 0 || rank >= world) return fail(c, DPMM_EINVAL, "bad rank / world");
    Rccl &r = rccl();
    if (!r.handle || !r.err.empty()) return fail(c, DPMM_ECOMM, r.err.empty() ? "RCCL unavailable" : r.err);
    HIPCHK(c, hipSetDevice(c->device));
    comm_release(c);
    UidByValue id;
    memcpy(id.internal, unique_id128, 128);
    void *comm = nullptr;
    const int rc = r.CommInitRank(&comm, world, id, rank);
    if (rc != 0) return fail(c, DPMM_ECOMM, std::string("ncclCommInitRank: ") + r.GetErrorString(rc));
    c->comm = comm; c->rank = rank; c->world = world;
    watchdog_start(c);
    return DPMM_OK;
}

int dpmm_comm_init_host(dpmm_ctx *c, int rank, int world, dpmm_host_allreduce_fn fn, void *user) {
    if (!c || !fn) return DPMM_EINVAL;
    if (world < 1 || rank < 0 || rank >= world) return fail(c, DPMM_EINVAL, "bad rank / world");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_stream(c, c->stream));
    comm_release(c);
    c->host_fn = fn; c->host_user = user; c->rank = rank; c->world = world;
    return DPMM_OK;
}

int dpmm_comm_info(dpmm_ctx *c, int64_t *out8) {
    if (!c || !out8) return DPMM_EINVAL;
    out8[0] = c->world; out8[1] = c->rank;
    out8[2] = c->comm ? 1 : (c->host_fn ? 2 : 0);
    out8[3] = c->comm_bytes[0]; out8[4] = c->comm_bytes[1]; out8[5] = c->comm_calls;
    out8[6] = 0;
    out8[7] = c->last_pass_one_collective ? 1 : 0;      // the last per-step pass used ONE collective (DPMM_OPT_ONE_COLLECTIVE)
    return DPMM_OK;
}

int dpmm_last_comm_ms(dpmm_ctx *c, float *counts_ms, float *rows_ms) {
    if (!c) return DPMM_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_stream(c, c->stream));
    if (counts_ms) { *counts_ms = 0.f; if (c->have_comm_ev[0]) HIPCHK(c, hipEventElapsedTime(counts_ms, c->ev_comm[0], c->ev_comm[1])); }
    if (rows_ms) { *rows_ms = 0.f; if (c->have_comm_ev[1]) HIPCHK(c, hipEventElapsedTime(rows_ms, c->ev_comm[2], c->ev_comm[3])); }
    return DPMM_OK;
}

int dpmm_comm_destroy(dpmm_ctx *c) {
    if (!c) return DPMM_EINVAL;
    hipSetDevice(c->device);
    if (c->stream && !c->comm_aborted.load()) sync_stream(c, c->stream);
    comm_release(c);
    return DPMM_OK;
}

int dpmm_comm_allgather_host(dpmm_ctx *c, const void *mine, int64_t bytes, void *all) {
    if (!c || !mine || !all || bytes < 0) return DPMM_EINVAL;
    if (!comm_attached(c) || c->world == 1) { memcpy(all, mine, (size_t)bytes); return DPMM_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nb = ((size_t)bytes + 7) & ~(size_t)7, tot = nb * (size_t)c->world;
    if (!c->comm) {
        // host transport: every rank contributes its piece in a zeroed [world][nb] buffer; the Int64 sum over the ranks is the gather
        std::vector<int64_t> buf(tot / 8, 0);
        memcpy(reinterpret_cast<char *>(buf.data()) + nb * (size_t)c->rank, mine, (size_t)bytes);
        const int hrc = c->host_fn(c->host_user, buf.data(), (int64_t)(tot / 8), 0);
        if (hrc != 0) return fail(c, DPMM_ECOMM, "host all-reduce callback failed (code " + std::to_string(hrc) + ")");
        for (int rk = 0; rk < c->world; ++rk) memcpy((char *)all + (size_t)rk * (size_t)bytes, reinterpret_cast<char *>(buf.data()) + nb * (size_t)rk, (size_t)bytes);
        return DPMM_OK;
    }
    if (int rc = ensure_pinned(c, nb + tot)) return rc;
    DevBuf<char> dbuf;
    HIPCHK(c, dbuf.alloc(tot));
    HIPCHK(c, sync_stream(c, c->stream));
    memcpy(c->h_pin, mine, (size_t)bytes);
    hipError_t e = launch_copy_bytes(dbuf + nb * (size_t)c->rank, c->h_pin, nb, c->stream);
    int rc = DPMM_OK;
    if (e == hipSuccess) {
        Rccl &r = rccl();
        const int nrc = r.AllGather(dbuf + nb * (size_t)c->rank, dbuf, nb, kNcclInt8, c->comm, c->stream);
        if (nrc != 0) rc = fail(c, DPMM_ECOMM, std::string("ncclAllGather: ") + r.GetErrorString(nrc));
    }
    if (rc == DPMM_OK && e == hipSuccess) e = launch_copy_bytes(c->h_pin + nb, dbuf, tot, c->stream);
    if (e == hipSuccess) e = sync_stream(c, c->stream);
    if (e != hipSuccess) { c->err = std::string("dpmm_comm_allgather_host: ") + hipGetErrorString(e); return DPMM_EHIP; }
    if (rc != DPMM_OK) return rc;
    for (int rk = 0; rk < c->world; ++rk) memcpy((char *)all + (size_t)rk * (size_t)bytes, c->h_pin + nb + nb * (size_t)rk, (size_t)bytes);
    return DPMM_OK;
}

// Sub-cluster log-likelihood table of the CURRENT parameters: out[(2k+s) * n_local + i] = loglik of point i under sub-cluster
// s of cluster k + log lr_weights[k][s] -- the two values create_subclusters_labels! (local_clusters_actions.jl:83-95) draws from
// for a point labelled k.  Same arithmetic as the sub-label phase of dpmm_sweep (the sub-cluster matrices are evaluated as
// the cluster-level rows of a temporary 2K-cluster parameter set, full table, no screening).
int dpmm_debug_subloglik(dpmm_ctx *c, float *out) {
    if (!c || !out) return DPMM_EINVAL;
    if (!c->have_points || !c->have_params || c->predictive) return fail(c, DPMM_ESTATE, "debug_subloglik needs points and sweep parameters");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0) return DPMM_OK;
    const int K = c->K, K2 = 2 * K;
    if (c->prior == DPMM_PRIOR_NIW && c->have_b3 && c->opt_b3 && c->have_tail && !c->predictive) {      // (the same condition as run_sweep's)
        // the sweeps' sub-label phase runs the three-plane bf16 evaluation (niw_lean.hip): the same device functions, for every point and cluster
        NiwSweepArgs a{};
        a.X = c->dX; a.ldx = c->ldx; a.n = c->n; a.K = K; a.mup = c->d_mup; a.cst = c->d_cst; a.tail = c->d_tail;
        DevBuf<float> tab;
        hipError_t e = tab.alloc(sizeof(float) * (size_t)K2 * (size_t)c->n);
        if (e == hipSuccess) e = launch_niw_b3_debug(a, tab, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(out, tab, sizeof(float) * (size_t)K2 * (size_t)c->n, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = sync_stream(c, c->stream);
        if (e != hipSuccess) { c->err = std::string("dpmm_debug_subloglik: ") + hipGetErrorString(e); return DPMM_EHIP; }
        return DPMM_OK;
    }
    if (c->prior == DPMM_PRIOR_MULT && c->x_sparse) {
        // the sparse sweep's table mode evaluates all 3K rows with the arithmetic of its sub-label phase: rows 3k + 1 + s are the answer
        const int64_t stride = c->ntiles * c->tile;
        DevBuf<float> table;
        HIPCHK(c, table.alloc(sizeof(float) * (size_t)(3 * K) * (size_t)stride));
        int rc = run_sweep(c, 0, 0, table, stride);
        hipError_t e = hipSuccess;
        for (int j = 0; j < K2 && rc == DPMM_OK && e == hipSuccess; ++j)
            e = hipMemcpyAsync(out + (size_t)j * c->n, table + (size_t)(3 * (j / 2) + 1 + (j % 2)) * stride, sizeof(float) * (size_t)c->n, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = sync_stream(c, c->stream);
        if (e != hipSuccess) { c->err = std::string("dpmm_debug_subloglik: ") + hipGetErrorString(e); return DPMM_EHIP; }
        return rc;
    }
    if (K2 > DPMM_MAX_CLUSTERS) return fail(c, DPMM_ELIMIT, "debug_subloglik: 2K > DPMM_MAX_CLUSTERS");
    const int64_t stride = c->ntiles * c->tile;
    const bool niw = c->prior == DPMM_PRIOR_NIW;
    // temporary parameter images: row 3j of the temporary set <- row 3k+1+s of the live one (j = 2k+s)
    const size_t NP = niw ? (size_t)c->NB * (c->NB + 1) / 2 : 0, matsz = NP * 256, dp = niw ? (size_t)16 * c->NB : 0;
    // the temporary images change places with the live ones for the sweep below and change back behind it
    DevBuf<float> tRp, tmu, tcst, table, traw;
    DevBuf<uint32_t> tL16;
    hipError_t e = tcst.alloc(sizeof(float) * 3 * K2);
    if (e == hipSuccess) e = table.alloc(sizeof(float) * (size_t)(niw ? K2 : 3 * K2) * (size_t)stride);
    int rc = DPMM_OK;
    const bool s_rp_current = c->rp_current;
    bool swapped = false;
    const int sK = c->K;
    const bool s_tail = c->have_tail, s_prep = c->have_screen_prep;
    if (e == hipSuccess && niw) {
        e = tRp.alloc(sizeof(float) * 3 * K2 * matsz);
        if (e == hipSuccess) e = tmu.alloc(sizeof(float) * 3 * K2 * dp);
        for (int j = 0; j < K2 && e == hipSuccess; ++j) {
            const int src = 3 * (j / 2) + 1 + (j % 2);
            e = hipMemcpyAsync(tRp + (size_t)(3 * j) * matsz, c->d_Rp + (size_t)src * matsz, sizeof(float) * matsz, hipMemcpyDeviceToDevice, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(tmu + (size_t)(3 * j) * dp, c->d_mup + (size_t)src * dp, sizeof(float) * dp, hipMemcpyDeviceToDevice, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(tcst + 3 * j, c->d_cst + src, sizeof(float), hipMemcpyDeviceToDevice, c->stream);
        }
        if (e == hipSuccess) { c->d_Rp.swap(tRp); c->d_mup.swap(tmu); c->d_cst.swap(tcst); swapped = true; }
    } else if (e == hipSuccess) {
        // Multinomial: re-pack a raw row image with the sub-cluster rows in the cluster-level positions
        e = traw.alloc(sizeof(float) * 3 * K2 * (size_t)c->ldx);
        if (e == hipSuccess) e = hipMemsetAsync(traw, 0, sizeof(float) * 3 * K2 * (size_t)c->ldx, c->stream);
        const size_t NT = (size_t)(c->ldx + 15) / 16, NRB = (size_t)(3 * K2 + 15) / 16;
        if (e == hipSuccess) e = tRp.alloc(sizeof(float) * NRB * NT * 256);
        if (e == hipSuccess) e = tL16.alloc(sizeof(uint32_t) * std::max(mult_pack_bf16_words(3 * K2, c->ldx), mult_pack_u8_words(3 * K2, (c->D + 127) / 128 * 128)));
        if (e == hipSuccess) e = hipMemsetAsync(tcst, 0, sizeof(float) * 3 * K2, c->stream);
        for (int j = 0; j < K2 && e == hipSuccess; ++j) {
            const int src = 3 * (j / 2) + 1 + (j % 2);
            e = hipMemcpyAsync(traw + (size_t)(3 * j) * c->ldx, c->d_raw + (size_t)src * c->ldx, sizeof(float) * c->ldx, hipMemcpyDeviceToDevice, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(tcst + 3 * j, c->d_cst + src, sizeof(float), hipMemcpyDeviceToDevice, c->stream);
        }
        if (e == hipSuccess) e = launch_mult_pack(traw, tRp, 3 * K2, c->ldx, c->stream);
        if (e == hipSuccess && c->x_u8) e = launch_mult_pack_u8(traw, tL16, 3 * K2, c->ldx, c->ld8, c->stream);
        else if (e == hipSuccess && c->x_bf16_exact) e = launch_mult_pack_bf16(traw, tL16, 3 * K2, c->ldx, c->stream);
        if (e == hipSuccess) { c->d_Rp.swap(tRp); c->d_cst.swap(tcst); c->d_Lp16.swap(tL16); c->d_raw.swap(traw); c->rp_current = true; swapped = true; }
    }
    if (e == hipSuccess) {
        c->K = K2; c->have_tail = false; c->have_screen_prep = false;
        rc = run_sweep(c, 0, 0, table, stride);
        if (rc == DPMM_OK) {
            const size_t src_pitch = sizeof(float) * stride * (niw ? 1 : 3);
            e = hipMemcpy2DAsync(out, sizeof(float) * c->n, table, src_pitch, sizeof(float) * c->n, (size_t)K2, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = sync_stream(c, c->stream);
        }
    }
    hipStreamSynchronize(c->stream);
    if (swapped) {
        c->d_Rp.swap(tRp); c->d_cst.swap(tcst);
        if (niw) c->d_mup.swap(tmu); else { c->d_Lp16.swap(tL16); c->d_raw.swap(traw); }
    }
    c->rp_current = s_rp_current; c->K = sK; c->have_tail = s_tail; c->have_screen_prep = s_prep;
    if (e != hipSuccess) { c->err = std::string("dpmm_debug_subloglik: ") + hipGetErrorString(e); return DPMM_EHIP; }
    return rc;
}

// Diagnostic for the reference bracket of the D <= 64 sweep (niw_sweep.hip, ref_bracket): q_hi[i] = the bracket's certified upper end of
// q_k(x_i) = |R_k (x_i - mu_k)|^2 for the cluster-level factor of `cluster` (1-based) and q[i] = the Float32 evaluation the sweep would
// make in its place -- same device functions and operand images as the sweep.  c_override > 0 replaces the library's rounding constant.
int dpmm_debug_ref_bracket(dpmm_ctx *c, int64_t cluster, float c_override, float *q_hi, float *q) {
    if (!c || !q_hi || !q) return DPMM_EINVAL;
    if (c->prior != DPMM_PRIOR_NIW || c->NB != 4) return fail(c, DPMM_ESTATE, "the reference bracket exists for the NIW prior with D in 33..64 only");
    if (!c->have_points || !c->have_params || c->predictive || !c->have_tail) return fail(c, DPMM_ESTATE, "debug_ref_bracket needs points and sweep parameters with tail records (D % 4 == 0, K > 2)");
    if (cluster < 1 || cluster > c->K) return fail(c, DPMM_EINVAL, "cluster index out of range");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0) return DPMM_OK;
    DevBuf<float> d;
    HIPCHK(c, d.alloc(sizeof(float) * 2 * (size_t)c->n));
    NiwSweepArgs a{};
    a.X = c->dX; a.ldx = c->ldx; a.n = c->n; a.K = c->K; a.Rp = c->d_Rp; a.mup = c->d_mup; a.tail = c->d_tail;
    hipError_t e = launch_niw_refb_debug(a, (int)cluster - 1, c_override, d, d + c->n, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(q_hi, d, sizeof(float) * (size_t)c->n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(q, d + c->n, sizeof(float) * (size_t)c->n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = sync_stream(c, c->stream);
    if (e != hipSuccess) { c->err = std::string("dpmm_debug_ref_bracket: ") + hipGetErrorString(e); return DPMM_EHIP; }
    return DPMM_OK;
}

int dpmm_debug_pair_ball(dpmm_ctx *c, float *pd, float *sn) {
    if (!c || !pd || !sn) return DPMM_EINVAL;
    if (c->prior != DPMM_PRIOR_NIW || c->NB != 4) return fail(c, DPMM_ESTATE, "the pair-ball table exists for the NIW prior with D in 33..64 only");
    if (!c->have_params || !c->have_pb) return fail(c, DPMM_ESTATE, "no pair-ball table for the parameters on the device (DPMM_OPT_PAIR_BALL, 2 <= K <= 256, tail records)");
    HIPCHK(c, hipSetDevice(c->device));
    const float *t = c->d_tail + niw_pair_ball_offset((size_t)c->K);
    const size_t K = (size_t)c->K;
    HIPCHK(c, hipMemcpyAsync(pd, t, sizeof(float) * K * K, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(sn, t + K * K, sizeof(float) * K, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, sync_stream(c, c->stream));
    return DPMM_OK;
}

int dpmm_debug_pair_ball_sn2(dpmm_ctx *c, float *sn2) {
    if (!c || !sn2) return DPMM_EINVAL;
    if (c->prior != DPMM_PRIOR_NIW || c->NB != 4) return fail(c, DPMM_ESTATE, "the pair-ball table exists for the NIW prior with D in 33..64 only");
    if (!c->have_params || !c->have_pb) return fail(c, DPMM_ESTATE, "no pair-ball table for the parameters on the device (DPMM_OPT_PAIR_BALL, 2 <= K <= 256, tail records)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t K = (size_t)c->K;
    HIPCHK(c, hipMemcpyAsync(sn2, c->d_tail + niw_pair_ball_offset(K) + K * K + K, sizeof(float) * K, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, sync_stream(c, c->stream));
    return DPMM_OK;
}

int dpmm_debug_norm_cert_points(dpmm_ctx *c, int enable, uint8_t *flags) {
    if (!c) return DPMM_EINVAL;
    if (c->prior != DPMM_PRIOR_NIW || c->NB != 4) return fail(c, DPMM_ESTATE, "the norm certificate exists for the NIW prior with D in 33..64 only");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_stream(c, c->stream));
    const size_t nb = ((size_t)std::max<int64_t>(c->n, 1) + 7) & ~(size_t)7;
    if (flags) {
        if (!c->d_cert_rec) return fail(c, DPMM_ESTATE, "dpmm_debug_norm_cert_points: the record is not switched on");
        HIPCHK(c, hipMemcpy(flags, c->d_cert_rec, (size_t)c->n, hipMemcpyDeviceToHost));
    }
    if (enable) {
        if (!c->d_cert_rec || c->d_cert_rec.bytes != nb) HIPCHK(c, c->d_cert_rec.alloc(nb));
        HIPCHK(c, hipMemset(c->d_cert_rec, 0, nb));
    } else c->d_cert_rec.reset();
    return DPMM_OK;
}

int dpmm_debug_bracket_big(dpmm_ctx *c, float *aref, uint32_t *tile_flags) {
    if (!c || !aref || !tile_flags) return DPMM_EINVAL;
    if (c->prior != DPMM_PRIOR_NIW || (c->NB != 8 && c->NB != 16)) return fail(c, DPMM_ESTATE, "this bracket exists for the NIW prior with D = 65 .. 256 only");
    if (!c->have_points || !c->have_params || c->predictive || !c->have_refb_big || !c->have_labels)
        return fail(c, DPMM_ESTATE, "debug_bracket_big needs points, labels and sweep parameters with tail records (D % 4 == 0, K > 2, DPMM_OPT_REF_BRACKET on)");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0) return DPMM_OK;
    const size_t nt = (size_t)((c->n + 127) / 128);
    DevBuf<float> d; DevBuf<uint32_t> f;
    HIPCHK(c, d.alloc(sizeof(float) * nt * 128));
    HIPCHK(c, f.alloc(sizeof(uint32_t) * nt));
    NiwSweepArgs a{};
    a.X = c->dX; a.ldx = c->ldx; a.n = c->n; a.K = c->K; a.mup = c->d_mup; a.cst = c->d_cst; a.bins = c->dbins;
    a.order = (c->have_perm && c->opt_ordered) ? c->sb.perm : nullptr; a.order_total = c->sb.perm_total;
    hipError_t e = hipMemsetAsync(d, 0, sizeof(float) * nt * 128, c->stream);
    if (e == hipSuccess) e = launch_niw_bracket_big(c->NB, a, c->d_refb_big, f, d, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(aref, d, sizeof(float) * (size_t)c->n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(tile_flags, f, sizeof(uint32_t) * nt, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = sync_stream(c, c->stream);
    if (e != hipSuccess) { c->err = std::string("dpmm_debug_bracket_big: ") + hipGetErrorString(e); return DPMM_EHIP; }
    return DPMM_OK;
}

int dpmm_last_sweep_parts_ms(dpmm_ctx *c, float *out3) {
    if (!c || !out3) return DPMM_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    out3[0] = out3[1] = out3[2] = 0.f;
    if (!c->have_sweep_ev || c->have_parts == 0) return DPMM_OK;
    HIPCHK(c, hipEventSynchronize(c->ev[1]));
    if (c->have_parts == 2) {
        HIPCHK(c, hipEventElapsedTime(&out3[0], c->ev[0], c->ev_part[0]));
        HIPCHK(c, hipEventElapsedTime(&out3[1], c->ev_part[0], c->ev_part[1]));
    } else HIPCHK(c, hipEventElapsedTime(&out3[1], c->ev[0], c->ev_part[1]));
    HIPCHK(c, hipEventElapsedTime(&out3[2], c->ev_part[1], c->ev[1]));
    return DPMM_OK;
}

int dpmm_last_kernel_ms(dpmm_ctx *c, float *sweep_ms, float *stats_ms) {
    if (!c) return DPMM_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    // wait for the closing event of each pair only (not for the stream: the draws launched ahead behind the posteriors are still running when
    // the engine reads the times of the step that just ended, and a stream synchronise here would put them on the host's critical path)
    if (sweep_ms) { *sweep_ms = 0.f; if (c->have_sweep_ev) { HIPCHK(c, hipEventSynchronize(c->ev[1])); HIPCHK(c, hipEventElapsedTime(sweep_ms, c->ev[0], c->ev[1])); } }
    if (stats_ms) { *stats_ms = 0.f; if (c->have_stats_ev) { HIPCHK(c, hipEventSynchronize(c->ev[3])); HIPCHK(c, hipEventElapsedTime(stats_ms, c->ev[2], c->ev[3])); } }
    return DPMM_OK;
}

// ---- include/dpmm_hip_tensor.h: caller-owned device memory in and out --------------------------------------------------------------
// Without a context there is nothing to work on: DPMM_ENODEVICE where no device exists (no CPU fallback), else a plain bad argument.
static int tensor_no_ctx(const char *fn) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(nullptr, DPMM_ENODEVICE, std::string(fn) + ": no HIP device available (this library has no CPU fallback)");
    }
    return fail(nullptr, DPMM_EINVAL, std::string(fn) + ": ctx is null");
}

// `bytes` from `p` must be device memory of the ctx's device, inside one allocation, aligned to `align`: checked with the two runtime queries
// before any launch (a bad pointer is a DPMM_EINVAL, never a GPU fault).  bytes == 0: nothing will be addressed, nothing to check.
static int check_device_extent(dpmm_ctx *c, const char *fn, const char *arg, const void *p, uint64_t bytes, size_t align) {
    const std::string who = std::string(fn) + ": " + arg;
    if (bytes == 0) return DPMM_OK;
    if (!p) return fail(c, DPMM_EINVAL, who + " is null");
    if (reinterpret_cast<uintptr_t>(p) % align) return fail(c, DPMM_EINVAL, who + " is not aligned to its element size (" + std::to_string(align) + " bytes)");
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, DPMM_EINVAL, who + " is not a device pointer (unknown to the HIP runtime)");
    }
    if (at.type != hipMemoryTypeDevice) return fail(c, DPMM_EINVAL, who + " is not device memory (host, managed or unregistered memory)");
    if (at.device != c->device) return fail(c, DPMM_EINVAL, who + " lives on device " + std::to_string(at.device) + ", the context on device " + std::to_string(c->device));
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(p)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, DPMM_EINVAL, who + ": the allocation it belongs to cannot be determined");
    }
    const uintptr_t b = reinterpret_cast<uintptr_t>(base), a = reinterpret_cast<uintptr_t>(p);
    if (a < b || a - b > size || bytes > size - (a - b))
        return fail(c, DPMM_EINVAL, who + ": the call addresses " + std::to_string((unsigned long long)bytes) + " bytes from it, its allocation holds " +
                                        std::to_string((unsigned long long)(a >= b && a - b <= size ? size - (a - b) : 0)));
    return DPMM_OK;
}

// a * b + ... in elements, refusing what does not fit 62 bits (the byte count must fit a uint64_t)
static bool extent_elems(int64_t n, int64_t sp, int D, int64_t sf, uint64_t *out) {
    const unsigned __int128 e = (unsigned __int128)(uint64_t)(n - 1) * (uint64_t)sp + (unsigned __int128)(uint64_t)(D - 1) * (uint64_t)sf + 1;
    if (e >> 58) return false;
    *out = (uint64_t)e;
    return true;
}

int dpmm_upload_points_strided_device(dpmm_ctx *c, const void *d_src, int dtype, int64_t stride_point, int64_t stride_feature, int nan_to_zero) {
    static const char *fn = "dpmm_upload_points_strided_device";
    if (!c) return tensor_no_ctx(fn);
    const size_t es = ingest_elem_size(dtype);
    if (es == 0) return fail(c, DPMM_EINVAL, std::string(fn) + ": dtype " + std::to_string(dtype) + " is not a DPMM_DT_* code");
    if (stride_point < 0 || stride_feature < 0) return fail(c, DPMM_EINVAL, std::string(fn) + ": stride_point / stride_feature is negative");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n > 0) {
        uint64_t elems = 0;
        if (!extent_elems(c->n, stride_point, c->D, stride_feature, &elems)) return fail(c, DPMM_EINVAL, std::string(fn) + ": the strides address more than 2^58 elements");
        if (int rc = check_device_extent(c, fn, "d_src", d_src, elems * es, es)) return rc;
    }
    // from here on as upload_common: the ctx-owned image, then what a Multinomial context derives from it
    if (int rc = ensure_points_buffer(c)) return rc;
    if (c->n > 0) {
        HIPCHK(c, launch_ingest_strided(c->dX, c->ldx, d_src, dtype, stride_point, stride_feature, c->n, c->D, nan_to_zero, c->stream));
        if (int rc = finish_upload(c)) return rc;
    }
    c->have_points = true;
    c->cache_force = true;
    c->rows_full_K = -1;
    return DPMM_OK;
}

// ---- include/dpmm_hip_project.h: wide points projected to the ctx's dimension while they are read (project.hip) --------------------
int dpmm_set_projection(dpmm_ctx *c, int D_in, const double *W, const double *mu) {
    static const char *fn = "dpmm_set_projection";
    if (!c) return tensor_no_ctx(fn);
    if (c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, std::string(fn) + ": ctx is not a NIW context (projections are for the NIW prior only)");
    if (D_in < 0) return fail(c, DPMM_EINVAL, std::string(fn) + ": D_in is negative");
    if (D_in > DPMM_MAX_DIM_PROJECT_IN) return fail(c, DPMM_ELIMIT, std::string(fn) + ": D_in > DPMM_MAX_DIM_PROJECT_IN");
    HIPCHK(c, hipSetDevice(c->device));
    if (D_in == 0) {
        HIPCHK(c, sync_stream(c, c->stream));
        c->d_proj_W.reset(); c->d_proj_bias.reset(); c->proj_Din = 0;
        return DPMM_OK;
    }
    if (!W) return fail(c, DPMM_EINVAL, std::string(fn) + ": W is null");
    std::vector<uint16_t> img;
    std::vector<float> bias;
    int64_t where = 0;
    if (const int bad = proj_build_image(D_in, c->D, proj_njb(c->D), W, mu, img, bias, &where)) {
        if (bad == 1) return fail(c, DPMM_EINVAL, std::string(fn) + ": W has a non-finite entry (or one beyond the Float32 / bf16 range) at [" + std::to_string(where / c->D) + "][" + std::to_string(where % c->D) + "]");
        if (bad == 2) return fail(c, DPMM_EINVAL, std::string(fn) + ": mu has a non-finite entry at [" + std::to_string(where) + "]");
        return fail(c, DPMM_EINVAL, std::string(fn) + ": mu' W overflows Float32 in column " + std::to_string(where));
    }
    DevBuf<void> dW;      // beside the projection in force, which stays when this fails
    DevBuf<float> db;
    hipError_t e = dW.alloc(img.size() * sizeof(uint16_t));
    if (e == hipSuccess) e = db.alloc(bias.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpyAsync(dW, img.data(), img.size() * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(db, bias.data(), bias.size() * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = sync_stream(c, c->stream);
    if (e != hipSuccess) return fail(c, DPMM_EHIP, std::string(fn) + ": " + hipGetErrorString(e));
    c->d_proj_W = std::move(dW); c->d_proj_bias = std::move(db); c->proj_Din = D_in;
    return DPMM_OK;
}

// the points in force become the projection of n_local points read from (device memory) src; everything was checked by the caller
static int upload_projected(dpmm_ctx *c, const void *src, int dtype, int64_t sp, int64_t sf, int64_t r0, int64_t nr) {
    HIPCHK(c, launch_project(c->dX + (size_t)r0 * c->ldx, c->ldx, c->D, src, dtype, sp, sf, nr, c->proj_Din, c->d_proj_W, c->d_proj_bias, c->stream));
    return DPMM_OK;
}

int dpmm_upload_points_projected_device(dpmm_ctx *c, const void *d_src, int dtype, int64_t stride_point, int64_t stride_feature) {
    static const char *fn = "dpmm_upload_points_projected_device";
    if (!c) return tensor_no_ctx(fn);
    if (c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, std::string(fn) + ": ctx is not a NIW context");
    if (c->proj_Din <= 0) return fail(c, DPMM_EINVAL, std::string(fn) + ": ctx has no projection (dpmm_set_projection)");
    const size_t es = ingest_elem_size(dtype);
    if (es == 0) return fail(c, DPMM_EINVAL, std::string(fn) + ": dtype " + std::to_string(dtype) + " is not a DPMM_DT_* code");
    if (stride_point < 0 || stride_feature < 0) return fail(c, DPMM_EINVAL, std::string(fn) + ": stride_point / stride_feature is negative");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n > 0) {
        uint64_t elems = 0;
        if (!extent_elems(c->n, stride_point, c->proj_Din, stride_feature, &elems)) return fail(c, DPMM_EINVAL, std::string(fn) + ": the strides address more than 2^58 elements");
        if (int rc = check_device_extent(c, fn, "d_src", d_src, elems * es, es)) return rc;
    }
    if (int rc = ensure_points_buffer(c)) return rc;
    if (c->n > 0) {
        if (int rc = upload_projected(c, d_src, dtype, stride_point, stride_feature, 0, c->n)) return rc;
        if (int rc = finish_upload(c)) return rc;
    }
    c->have_points = true;
    c->cache_force = true;
    c->rows_full_K = -1;
    return DPMM_OK;
}

int dpmm_upload_points_projected(dpmm_ctx *c, const float *h_src, int64_t ld_src) {
    static const char *fn = "dpmm_upload_points_projected";
    if (!c) return tensor_no_ctx(fn);
    if (c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, std::string(fn) + ": ctx is not a NIW context");
    if (c->proj_Din <= 0) return fail(c, DPMM_EINVAL, std::string(fn) + ": ctx has no projection (dpmm_set_projection)");
    if (!h_src && c->n > 0) return fail(c, DPMM_EINVAL, std::string(fn) + ": h_src is null");
    if (ld_src < c->proj_Din) return fail(c, DPMM_EINVAL, std::string(fn) + ": ld_src < D_in");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_points_buffer(c)) return rc;
    if (c->n > 0) {
        // compact rows [chunk][D_in] in one buffer of at most 64 MiB, kept for the next call
        const size_t row_bytes = sizeof(float) * (size_t)c->proj_Din;
        const int64_t chunk_rows = std::max<int64_t>(1, std::min<int64_t>(c->n, (int64_t)(((size_t)64 << 20) / row_bytes)));
        const size_t need = row_bytes * (size_t)chunk_rows;
        if (int rc = grow(c, c->d_proj_stage, need, fn, "staging rows")) return rc;
        for (int64_t r0 = 0; r0 < c->n; r0 += chunk_rows) {
            const int64_t nr = std::min(chunk_rows, c->n - r0);
            HIPCHK(c, hipMemcpy2DAsync(c->d_proj_stage, row_bytes, h_src + (size_t)r0 * (size_t)ld_src, sizeof(float) * (size_t)ld_src, row_bytes, (size_t)nr,
                                       hipMemcpyHostToDevice, c->stream));
            if (int rc = upload_projected(c, c->d_proj_stage, DPMM_DT_F32, c->proj_Din, 1, r0, nr)) return rc;
            HIPCHK(c, sync_stream(c, c->stream));          // the staging rows are reused by the next chunk
        }
        if (int rc = finish_upload(c)) return rc;
    }
    c->have_points = true;
    c->cache_force = true;
    c->rows_full_K = -1;
    return DPMM_OK;
}

// ---- include/dpmm_hip_csc.h: sparse points out of caller-owned device memory (csc_io.hip).  Between the phases the host reads the
// 8-byte word of the first offender and the 8-byte number of entries kept; temporary memory is cnt [n] and the scan's tile totals.
int dpmm_upload_points_csc_device(dpmm_ctx *c, const void *d_colptr, int index_dtype, const void *d_rowval, const void *d_nzval, int value_dtype,
                                  int64_t nnz_extent, int index_base) {
    static const char *fn = "dpmm_upload_points_csc_device";
    const std::string who = std::string(fn) + ": ";
    if (!c) return tensor_no_ctx(fn);
    if (c->prior != DPMM_PRIOR_MULT) return fail(c, DPMM_EINVAL, who + "sparse points are for Multinomial contexts");
    if (c->D > DPMM_MAX_DIM_MULT_SPARSE) return fail(c, DPMM_ELIMIT, who + "D > DPMM_MAX_DIM_MULT_SPARSE");
    if (index_dtype != DPMM_DT_I32 && index_dtype != DPMM_DT_I64)
        return fail(c, DPMM_EINVAL, who + "index_dtype " + std::to_string(index_dtype) + " is neither DPMM_DT_I32 nor DPMM_DT_I64");
    const size_t is = ingest_elem_size(index_dtype), vs = ingest_elem_size(value_dtype);
    if (vs == 0) return fail(c, DPMM_EINVAL, who + "value_dtype " + std::to_string(value_dtype) + " is not a DPMM_DT_* code");
    if (index_base != 0 && index_base != 1) return fail(c, DPMM_EINVAL, who + "index_base must be 0 or 1");
    if (nnz_extent < 0 || (nnz_extent >> 58)) return fail(c, DPMM_EINVAL, who + "nnz_extent out of range");
    if (index_dtype == DPMM_DT_I32 && nnz_extent + index_base > INT32_MAX) return fail(c, DPMM_EINVAL, who + "nnz_extent does not fit Int32 offsets");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = c->n;
    if (n > 0) {
        if (int rc = check_device_extent(c, fn, "d_colptr", d_colptr, ((uint64_t)n + 1) * is, is)) return rc;
        if (int rc = check_device_extent(c, fn, "d_rowval", d_rowval, (uint64_t)nnz_extent * is, is)) return rc;
        if (int rc = check_device_extent(c, fn, "d_nzval", d_nzval, (uint64_t)nnz_extent * vs, vs)) return rc;
    }
    // everything is built beside the points in force; they are replaced only when the new ones have passed the checks
    DevBuf<int64_t> n_cp, t_bt;
    DevBuf<float> n_val;
    DevBuf<uint16_t> n_ri;
    DevBuf<int32_t> t_cnt;
    const int64_t ntiles = csc_scan_tiles(n);
    unsigned long long bad = ~0ull;
    int64_t kept = 0;
    hipError_t e = n_cp.alloc(sizeof(int64_t) * ((size_t)n + 1));
    if (e == hipSuccess && n > 0) {
        unsigned long long *t_bad = nullptr;
        e = t_cnt.alloc(sizeof(int32_t) * (size_t)n);
        if (e == hipSuccess) e = t_bt.alloc(sizeof(int64_t) * ((size_t)ntiles + 2));       // tile totals, the sum of all, the first offender
        if (e == hipSuccess) {
            t_bad = reinterpret_cast<unsigned long long *>(t_bt + ntiles + 1);
            e = hipMemsetAsync(t_bad, 0xFF, sizeof(unsigned long long), c->stream);
        }
        if (e == hipSuccess) e = launch_csc_dev_check(d_colptr, d_rowval, d_nzval, index_dtype == DPMM_DT_I64, value_dtype, n, nnz_extent, c->D, index_base,
                                                      t_cnt, t_bad, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, t_bad, sizeof(bad), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = sync_stream(c, c->stream);
        if (e == hipSuccess && bad == ~0ull) {
            e = launch_csc_scan(t_cnt, n, t_bt, n_cp, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(&kept, t_bt + ntiles, sizeof(kept), hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = sync_stream(c, c->stream);
            const size_t nn = (size_t)std::max<int64_t>(kept, 1);
            if (e == hipSuccess) e = n_ri.alloc(sizeof(uint16_t) * nn);
            if (e == hipSuccess) e = n_val.alloc(sizeof(float) * nn);
            if (e == hipSuccess) e = launch_csc_dev_compact(d_colptr, d_rowval, d_nzval, index_dtype == DPMM_DT_I64, value_dtype, n, index_base, n_cp, n_ri,
                                                            n_val, c->stream);
            if (e == hipSuccess) e = sync_stream(c, c->stream);
        }
    } else if (e == hipSuccess) {
        e = hipMemsetAsync(n_cp, 0, sizeof(int64_t), c->stream);
        if (e == hipSuccess) e = sync_stream(c, c->stream);
    }
    if (e != hipSuccess || bad != ~0ull) {
        if (e != hipSuccess) return fail(c, DPMM_EHIP, who + hipGetErrorString(e));
        const std::string pt = std::to_string((long long)(bad >> 20));
        switch ((int)(bad & 7)) {
            case CSC_BAD_RANGE: return fail(c, DPMM_EINVAL, who + "point " + pt + ": row index out of range");
            case CSC_BAD_ORDER: return fail(c, DPMM_EINVAL, who + "point " + pt + ": row indices are not strictly increasing (unsorted or duplicate)");
            case CSC_BAD_DECREASES: return fail(c, DPMM_EINVAL, who + "colptr decreases at point " + pt);
            default: return fail(c, DPMM_EINVAL, who + "colptr points outside rowval / nzval at point " + pt);
        }
    }
    // from here on as dpmm_upload_points_csc
    t_cnt.reset(); t_bt.reset();      // (before set_points_chunk sizes the slabs)
    c->dX.reset(); c->dX8.reset();
    c->d_cp = std::move(n_cp); c->d_ri = std::move(n_ri); c->d_val = std::move(n_val); c->nnz = kept;
    c->x_sparse = 1; c->x_u8 = 0; c->x_bf16_exact = 0; c->repack_pending = false;
    if (int rc2 = set_points_chunk(c, true)) return rc2;
    if (c->have_params && c->d_raw) {
        if (int rc2 = pack_sparse_image(c, c->d_raw, c->d_Rp, c->K)) return rc2;
        c->rp_current = false;
        c->mspec_valid = false;
        HIPCHK(c, sync_stream(c, c->stream));
    }
    c->have_points = true;
    c->cache_force = true;
    c->rows_full_K = -1;
    return DPMM_OK;
}

int dpmm_get_points_device(dpmm_ctx *c, float *d_out, int64_t ld_out) {
    static const char *fn = "dpmm_get_points_device";
    if (!c) return tensor_no_ctx(fn);
    if (!c->have_points) return fail(c, DPMM_ESTATE, std::string(fn) + ": no points uploaded");
    if (ld_out < c->D) return fail(c, DPMM_EINVAL, std::string(fn) + ": ld_out < D");
    if (ld_out >> 40) return fail(c, DPMM_EINVAL, std::string(fn) + ": ld_out out of range");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0) return DPMM_OK;
    if (int rc = check_device_extent(c, fn, "d_out", d_out, (uint64_t)c->n * (uint64_t)ld_out * sizeof(float), sizeof(float))) return rc;
    if (c->x_sparse) {
        HIPCHK(c, launch_points_readback(d_out, ld_out, nullptr, 0, nullptr, 0, c->n, c->D, c->stream));
        HIPCHK(c, launch_sparse_readback(d_out, ld_out, c->d_cp, c->d_ri, c->d_val, c->n, c->stream));
    } else if (c->dX) {
        HIPCHK(c, launch_points_readback(d_out, ld_out, c->dX, c->ldx, nullptr, 0, c->n, c->D, c->stream));
    } else if (c->x_u8 && c->dX8) {
        HIPCHK(c, launch_points_readback(d_out, ld_out, nullptr, 0, c->dX8, c->ld8, c->n, c->D, c->stream));
    } else return fail(c, DPMM_ESTATE, std::string(fn) + ": the context holds no point storage");
    HIPCHK(c, sync_stream(c, c->stream));
    return DPMM_OK;
}

int dpmm_get_labels_device(dpmm_ctx *c, int64_t *d_labels, int64_t *d_sub) {
    static const char *fn = "dpmm_get_labels_device";
    if (!c) return tensor_no_ctx(fn);
    if (!c->have_labels) return fail(c, DPMM_ESTATE, "labels not initialised");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0 || (!d_labels && !d_sub)) return DPMM_OK;
    const uint64_t bytes = sizeof(int64_t) * (uint64_t)c->n;
    if (d_labels) if (int rc = check_device_extent(c, fn, "d_labels", d_labels, bytes, sizeof(int64_t))) return rc;
    if (d_sub) if (int rc = check_device_extent(c, fn, "d_sub", d_sub, bytes, sizeof(int64_t))) return rc;
    HIPCHK(c, launch_bins_to_i64(c->dbins, d_labels, d_sub, c->n, c->stream));      // (writes only the vectors that are given)
    HIPCHK(c, sync_stream(c, c->stream));
    return DPMM_OK;
}

int dpmm_set_labels_device(dpmm_ctx *c, const int64_t *d_labels, const int64_t *d_sub) {
    static const char *fn = "dpmm_set_labels_device";
    if (!c) return tensor_no_ctx(fn);
    if (!c->have_labels && (!d_labels || !d_sub)) return fail(c, DPMM_ESTATE, "first dpmm_set_labels_device must provide both vectors");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0) { c->have_labels = true; return DPMM_OK; }
    const uint64_t bytes = sizeof(int64_t) * (uint64_t)c->n;
    if (d_labels) if (int rc = check_device_extent(c, fn, "d_labels", d_labels, bytes, sizeof(int64_t))) return rc;
    if (d_sub) if (int rc = check_device_extent(c, fn, "d_sub", d_sub, bytes, sizeof(int64_t))) return rc;
    if (d_labels || d_sub) {
        HIPCHK(c, launch_bins_from_i64(c->dbins, d_labels, d_sub, c->n, c->stream));
        HIPCHK(c, sync_stream(c, c->stream));
    }
    c->have_labels = true;
    c->rows_full_K = -1;
    return DPMM_OK;
}

int dpmm_predict_points_device(dpmm_ctx *c, int64_t *d_labels, float *d_probs) {
    static const char *fn = "dpmm_predict_points_device";
    if (!c) return tensor_no_ctx(fn);
    if (!c->predictive) return fail(c, DPMM_ESTATE, "dpmm_predict_points_device needs dpmm_set_predictive_* first");
    if (!c->have_points || !c->have_params) return fail(c, DPMM_ESTATE, "predict needs points and parameters");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0) return DPMM_OK;
    if (!d_labels) return fail(c, DPMM_EINVAL, std::string(fn) + ": d_labels is null");
    if (int rc = check_device_extent(c, fn, "d_labels", d_labels, sizeof(int64_t) * (uint64_t)c->n, sizeof(int64_t))) return rc;
    if (d_probs) if (int rc = check_device_extent(c, fn, "d_probs", d_probs, sizeof(float) * (uint64_t)c->n * (uint64_t)c->K, sizeof(float))) return rc;
    const int64_t stride = c->ntiles * c->tile;
    const int rstep = (c->prior == DPMM_PRIOR_NIW) ? 1 : 3;       // Multinomial: rows 3k are the cluster-level rows
    DevBuf<float> table;
    HIPCHK(c, table.alloc(sizeof(float) * (size_t)(rstep * c->K) * (size_t)stride));
    int rc = run_sweep(c, 0, 0, table, stride);
    if (rc == DPMM_OK) {
        hipError_t e = launch_predict_finish(table, stride, rstep, c->n, c->K, d_labels, d_probs, c->stream);
        if (e == hipSuccess) e = sync_stream(c, c->stream);
        if (e != hipSuccess) { c->err = std::string(fn) + ": " + hipGetErrorString(e); rc = DPMM_EHIP; }
    }
    return rc;
}

// ---- include/dpmm_hip_score.h: log-density, top-m, labels and probabilities, slab by slab ----------------------------------------------
// slabs of whole tiles: as many as the budget holds, one at least; the ctx's table is grown to one slab.  rstep: cluster k is row k * rstep;
// P: points of a slab = floats between two rows of the table
static int score_table_slab(dpmm_ctx *c, int *rstep_out, int64_t *P_out) {
    const int rstep = (c->prior == DPMM_PRIOR_NIW) ? 1 : 3;       // Multinomial: rows 3k are the cluster-level rows
    const size_t rows = (size_t)rstep * (size_t)c->K;
    const double tile_bytes = (double)rows * (double)c->tile * sizeof(float);
    int64_t slab_tiles = (int64_t)std::min<double>(std::floor(c->opt_score_mb * 1048576.0 / tile_bytes), (double)c->ntiles);
    if (slab_tiles < 1) slab_tiles = 1;
    const int64_t P = slab_tiles * c->tile;
    *rstep_out = rstep; *P_out = P;
    return grow(c, c->d_score_table, sizeof(float) * rows * (size_t)P, "dpmm_score_points", "table");
}


// ---- include/dpmm_hip_missing.h: the marginal entries of points with NaN features, range by range (missing.hip) ---------------------------
// The device copies that missing.hip and typicality.hip read -- the transposed factors Rt and the constants [K][MISS_CST] -- are those of the
// predictive set in force afterwards.
static int miss_params(dpmm_ctx *c, const char *fn) {
    const std::string who = std::string(fn) + ": ";
    if (c->prior != DPMM_PRIOR_NIW || c->h_miss_cst.size() != (size_t)c->K * MISS_CST || !c->d_par)
        return fail(c, DPMM_ESTATE, who + "missing features need dpmm_set_predictive_niw");
    const size_t K = (size_t)c->K, D = (size_t)c->D;
    if (c->miss_gen != c->pred_gen) {
        if (int rc = grow(c, c->d_miss_rt, sizeof(float) * K * D * (size_t)miss_pitch(c->D), "dpmm_score_points", "transposed factors of the missing-feature pass")) return rc;
        if (int rc = grow(c, c->d_miss_cst, sizeof(double) * K * MISS_CST, "dpmm_score_points", "constants of the missing-feature pass")) return rc;
        HIPCHK(c, sync_stream(c, c->stream));
        HIPCHK(c, hipMemcpy(c->d_miss_cst, c->h_miss_cst.data(), sizeof(double) * K * MISS_CST, hipMemcpyHostToDevice));
        const ParLayout L = par_layout(c, c->miss_slots);
        const float *Rpk = reinterpret_cast<const float *>(c->d_par + (L.mat - L.cst));      // cluster k: row 3k of the staging image (identity slot map)
        HIPCHK(c, launch_miss_transpose(Rpk, 3 * (int64_t)(D * (D + 1) / 2), c->d_miss_rt, c->K, c->D, c->stream));
        c->miss_gen = c->pred_gen;
    }
    return DPMM_OK;
}

// The result of a table call's launches and copies as its return code (an int is one already)
static int table_result(dpmm_ctx *c, const char *fn, hipError_t e) {
    if (e != hipSuccess) { c->err = std::string(fn) + ": " + hipGetErrorString(e); return DPMM_EHIP; }
    return DPMM_OK;
}
static int table_result(dpmm_ctx *, const char *, int rc) { return rc; }

extern "C++" {      // down to the staging of the outputs: the templates among these helpers cannot have the C linkage of the block around them
// What MissArgs and TypicalityArgs share: one range of the table (np points from point p0, rows P floats apart), its points, miss_params' copies
template <class Args>
static Args niw_range_args(dpmm_ctx *c, int64_t P, int64_t p0, int64_t np) {
    const ParLayout L = par_layout(c, c->miss_slots);
    Args a{};
    a.table = c->d_score_table; a.stride = P; a.n = np; a.K = c->K; a.D = c->D;
    a.X = c->dX + p0 * c->ldx; a.ldx = c->ldx;
    a.Rt = c->d_miss_rt; a.mu = reinterpret_cast<const float *>(c->d_par + (L.mu - L.cst)); a.mu_step = 3 * (int64_t)c->D;
    a.cst = c->d_miss_cst;
    return a;
}

// Called once per table call, behind score_table_slab.  on: the call marginalises -- the device buffers exist afterwards (the list sized for
// one range of P points), the copies of the parameters are those of the predictive set in force, the per-call counters are cleared.
static int miss_begin(dpmm_ctx *c, bool on, int64_t P, const char *fn) {
    c->miss_counted = false;
    if (!on) return DPMM_OK;
    if (int rc = grow(c, c->d_miss_cnt, 3 * sizeof(unsigned long long), "dpmm_score_points", "counters of the missing-feature pass")) return rc;
    if (int rc = grow(c, c->d_miss_list, sizeof(uint32_t) * (size_t)P, "dpmm_score_points", "list of the missing-feature pass")) return rc;
    if (int rc = miss_params(c, fn)) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_miss_cnt, 0, 3 * sizeof(unsigned long long), c->stream));
    c->miss_counted = true;
    return DPMM_OK;
}

// One range of the table (np points from point p0, rows P floats apart), just evaluated on the ctx stream: list, then patch.  out != null
// (rows of the range's points, ld floats apart): the imputation behind them.
static int miss_range(dpmm_ctx *c, int64_t P, int64_t p0, int64_t np, float *out, int64_t ld, const char *fn) {
    MissArgs a = niw_range_args<MissArgs>(c, P, p0, np);
    a.list = c->d_miss_list; a.cnt = c->d_miss_cnt; a.out = out; a.ld_out = ld;
    hipError_t e = hipMemsetAsync(c->d_miss_cnt, 0, sizeof(unsigned long long), c->stream);
    if (e == hipSuccess) e = launch_miss_list(a, c->stream);
    if (e == hipSuccess) e = launch_miss_patch(a, false, 8 * c->cus, c->stream);
    if (e == hipSuccess && out) e = launch_miss_patch(a, true, 8 * c->cus, c->stream);
    return table_result(c, fn, e);
}

// ---- the walk every call over the score table makes: the table range by range, each range evaluated, patched where the call marginalises,
// and handed to the call's consumer.  A new scoring call plugs in here.
enum WalkMissing { WALK_MISS_NEVER, WALK_MISS_OPTION, WALK_MISS_ALWAYS };      // never (count data) | per DPMM_OPT_SCORE_MISSING | always (imputation)
struct TableWalk {
    int rstep = 0;       // cluster k is row k * rstep
    int64_t P = 0;       // points of a range = floats between two rows of the table
    bool miss = false;   // walk_ranges runs the missing-feature pass on every range
};

// The ctx's table grown to one range, then `size(P)` -- the refusals and per-range buffers of the call that go in front of the missing-feature
// pass -- then that pass made ready (miss_begin).
template <class Size>
static int walk_open(dpmm_ctx *c, const char *fn, WalkMissing missing, TableWalk *w, Size size) {
    if (int rc = score_table_slab(c, &w->rstep, &w->P)) return rc;
    if (int rc = size(w->P)) return rc;
    w->miss = missing == WALK_MISS_ALWAYS || (missing == WALK_MISS_OPTION && c->opt_score_missing != 0);
    return miss_begin(c, w->miss, w->P, fn);
}
static int walk_open(dpmm_ctx *c, const char *fn, WalkMissing missing, TableWalk *w) {
    return walk_open(c, fn, missing, w, [](int64_t) { return DPMM_OK; });
}

// The ranges that hold points 0 .. limit - 1 (limit = n_local for the per-point calls, n_valid for the accumulators), in order on the ctx
// stream.  consume(p0, np, nv) -> int or hipError_t: the call's own launches for the range at point p0; np points were evaluated, the first nv
// of them lie below the limit.
template <class Consume>
static int walk_ranges(dpmm_ctx *c, const TableWalk &w, int64_t limit, const char *fn, Consume consume) {
    for (int64_t p0 = 0; p0 < limit; p0 += w.P) {
        const int64_t np = std::min<int64_t>(w.P, c->n - p0);              // the range dpmm_score_points evaluates
        if (int rc = run_sweep(c, 0, 0, c->d_score_table, w.P, p0, np)) return rc;
        if (w.miss) if (int rc = miss_range(c, w.P, p0, np, nullptr, 0, fn)) return rc;
        if (int rc = table_result(c, fn, consume(p0, np, std::min<int64_t>(np, limit - p0)))) return rc;      // (nv: what of the range the call consumes)
    }
    return DPMM_OK;
}

// ---- the caller's arrays of a table call -- its outputs and, where a kernel reads one, a per-point input (`in`): used in place in the caller's
// device memory, or staged on the device and copied back to (inputs: in from) the caller's host memory.
// A column is the caller's pointer (null: not asked for), the argument's name in the messages, the size of its words and its bytes per
// element; in the staging buffer the columns follow each other in list order, each block 8-byte aligned.  A pitched column has rows: an
// element is `rows` rows of `bytes` bytes, `pitch` bytes apart at the caller's and dense in the staging buffer, and the words of the caller's
// rows behind `bytes` are written as zeros -- or, with `keep`, left as they are (host variant; the device variant's are the kernel's affair).
struct OutCol {
    void *dst;
    const char *name;
    size_t word;         // the alignment asked of dst
    size_t bytes;        // per element, or per row of a pitched column
    size_t pitch = 0;    // bytes between two rows at the caller's; 0: not pitched
    size_t rows = 1;     // rows per element of a pitched column (L for the quantiles)
    bool in = false;     // an input of the kernel: dst is read, by load()
    bool keep = false;   // flush writes nothing behind the rows
    size_t off = 0;
    size_t staged() const { return rows * bytes; }                      // bytes of an element in the staging buffer
    size_t step() const { return rows * (pitch ? pitch : bytes); }      // and at the caller's
};
template <int N>
struct OutStage {
    OutCol col[N];
    bool device;         // dst is device memory: nothing is staged
    bool every = false;  // the kernel writes every column, also those not asked for (dpmm_rank_read)
    char *buf = nullptr; // the staging buffer of layout(count) bytes
    // bytes of the staging buffer for `count` elements per column
    size_t layout(size_t count) {
        size_t total = 0;
        for (OutCol &q : col) { q.off = total; if (q.dst || every) total += (count * q.staged() + 7) & ~(size_t)7; }
        return total;
    }
    // device variant: `count` elements from every pointer given are device memory of the ctx's device, refused in list order
    int check(dpmm_ctx *c, const char *fn, uint64_t count) const {
        if (device)
            for (const OutCol &q : col)
                if (q.dst) if (int rc = check_device_extent(c, fn, q.name, q.dst, count * q.step(), q.word)) return rc;
        return DPMM_OK;
    }
    // host variant: the ctx's staging block grown to ranges of P points
    int open(dpmm_ctx *c, int64_t P) {
        if (device) return DPMM_OK;
        if (int rc = grow(c, c->d_score_out, layout((size_t)P), "dpmm_score_points", "staging of the outputs")) return rc;
        buf = c->d_score_out;
        return DPMM_OK;
    }
    // where the kernel writes (reads) column i for the elements from e0 on (null: not at all)
    template <class T>
    T *at(int i, int64_t e0) const {
        const OutCol &q = col[i];
        if (device) return q.dst ? reinterpret_cast<T *>(static_cast<char *>(q.dst) + (size_t)e0 * q.step()) : nullptr;
        return q.dst || every ? reinterpret_cast<T *>(buf + q.off) : nullptr;
    }
    // host variant, in front of the launch: `count` elements of every input column from the caller's element e0
    hipError_t load(dpmm_ctx *c, int64_t e0, size_t count) const {
        hipError_t e = hipSuccess;
        for (const OutCol &q : col)
            if (e == hipSuccess && q.dst && q.in)
                e = hipMemcpy2DAsync(buf + q.off, q.bytes, static_cast<char *>(q.dst) + (size_t)e0 * q.step(), q.pitch ? q.pitch : q.bytes, q.bytes, count * q.rows,
                                     hipMemcpyHostToDevice, c->stream);
        return e;
    }
    // host variant, behind the launch: `count` elements of every column asked for to the caller's element e0, in list order; then the wait,
    // since the blocks are rewritten by the next range; then the zeros behind the rows of the pitched columns that do not keep theirs
    hipError_t flush(dpmm_ctx *c, int64_t e0, size_t count) const {
        hipError_t e = hipSuccess;
        for (const OutCol &q : col) {
            if (e != hipSuccess || !q.dst || q.in) continue;
            char *dst = static_cast<char *>(q.dst) + (size_t)e0 * q.step();
            if (q.pitch && q.pitch != q.bytes) e = hipMemcpy2DAsync(dst, q.pitch, buf + q.off, q.bytes, q.bytes, count * q.rows, hipMemcpyDeviceToHost, c->stream);
            else e = hipMemcpyAsync(dst, buf + q.off, count * q.staged(), hipMemcpyDeviceToHost, c->stream);
        }
        if (e == hipSuccess) e = sync_stream(c, c->stream);
        for (const OutCol &q : col)
            if (e == hipSuccess && q.dst && !q.in && !q.keep && q.pitch > q.bytes)
                for (size_t r = (size_t)e0 * q.rows; r < ((size_t)e0 + count) * q.rows; ++r) memset(static_cast<char *>(q.dst) + r * q.pitch + q.bytes, 0, q.pitch - q.bytes);
        return e;
    }
};

// ---- the points of a call that take no part, counted per 32-point tile of a range by the kernels (regress_device.h, recommend.hip): one
// word per tile of a range of P points, ADDED to by the launches of every range
static int skip_open(dpmm_ctx *c, DevBuf<unsigned> &buf, int64_t P, const char *fn, const char *what) {
    const size_t bytes = sizeof(unsigned) * (size_t)((P + 31) / 32);
    if (int rc = grow(c, buf, bytes, fn, what)) return rc;
    HIPCHK(c, hipMemsetAsync(buf, 0, bytes, c->stream));
    return DPMM_OK;
}
// behind the last range: the wait for the ctx stream, then the words added up into skipped[0] (null: not asked for)
static int skip_close(dpmm_ctx *c, DevBuf<unsigned> &buf, int64_t P, int64_t *skipped) {
    HIPCHK(c, sync_stream(c, c->stream));
    if (!skipped) return DPMM_OK;
    std::vector<unsigned> cnt((size_t)((P + 31) / 32));
    HIPCHK(c, hipMemcpy(cnt.data(), buf, sizeof(unsigned) * cnt.size(), hipMemcpyDeviceToHost));
    int64_t total = 0;
    for (unsigned v : cnt) total += v;
    skipped[0] = total;
    return DPMM_OK;
}

// ---- what the calls of the mixture regression refuse first, in this order: no ctx, the prior, no predictive set, no tables for the set in
// force, then what the call needs beside the tables
enum RegressNeeds { REGRESS_TABLES, REGRESS_FACTOR, REGRESS_LEVELS };
static int regress_front(dpmm_ctx *c, const char *fn, RegressNeeds needs) {
    if (!c) return tensor_no_ctx(fn);
    c->miss_counted = false;      // (as score_points)
    const std::string who = std::string(fn) + ": ";
    if (c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, who + "the regression is that of the NIW prior's Student-t predictive");
    if (!c->predictive) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_predictive_niw first");
    if (c->reg_gen == 0 || c->reg_gen != c->pred_gen) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_regression for the predictive parameters in force");
    if (needs == REGRESS_FACTOR && !c->reg_factor) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_regression_factor for the regression tables in force");
    if (needs == REGRESS_LEVELS && (c->reg_lev_gen == 0 || c->reg_lev_gen != c->pred_gen))
        return fail(c, DPMM_ESTATE, who + "needs dpmm_set_regression_levels for the regression tables in force");
    return DPMM_OK;
}
// One range of the table (np points from point p0, rows P floats apart) and its points as the regression kernels take them
static RegressTile regress_tile(dpmm_ctx *c, int64_t P, int64_t p0, int64_t np, int64_t *labels, unsigned *skip) {
    RegressTile t{};
    t.table = c->d_score_table; t.stride = P; t.n = np; t.K = c->K; t.D = c->D; t.Dt = c->reg_Dt; t.Tp = regress_pitch(c->reg_Dt);
    t.X = c->dX + p0 * c->ldx; t.ldx = c->ldx;
    t.c = c->d_reg_c; t.hd = c->d_reg_hd; t.labels = labels; t.skip = skip;
    return t;
}
// the same fields of RegressCdfArgs and RegressQuantileArgs, which hold them flat (dpmm_kernels.h says why), and the tables beside them
template <class Args>
static Args regress_flat_args(dpmm_ctx *c, const RegressTile &t) {
    Args a{};
    a.table = t.table; a.stride = t.stride; a.n = t.n; a.K = t.K; a.D = t.D; a.Dt = t.Dt; a.Tp = t.Tp; a.X = t.X; a.ldx = t.ldx;
    a.c = t.c; a.hd = t.hd; a.labels = t.labels; a.skip = t.skip;
    a.Bt = c->d_reg_bt; a.V = c->d_reg_v;
    return a;
}

// ---- draws of every point (include/dpmm_hip_impute.h, include/dpmm_hip_regress_draw.h): element (jd, i, f) of the caller's at
// out[jd * draw_stride + i * ld + f], W floats of a row drawn (`wname` in the messages), the components at comp[jd * n_local + i].  Per
// range the draws go into the caller's device memory, or in batches of draws through the staging block ([batch][np][W] floats, then
// [batch][np] components), are copied back, and the words of the caller's rows behind W are written as zeros.
struct DrawDest {       // where a launch writes the draws j0 .. j0 + nb - 1 of a range
    float *out;
    int64_t ld, draw_stride;
    int32_t *comp;
    int64_t comp_stride;
};
struct DrawBatch {
    float *out;
    int64_t ld, draw_stride;
    int32_t *comp;
    int64_t ndraws;
    bool device;
    int64_t W;
    const char *wname;
    int64_t batch = 0, P = 0;
    // the refusals that need no device; cap: the draws a key holds, `capname` in the message
    int check(dpmm_ctx *c, const char *fn, int64_t i0, int64_t draw0, int64_t cap, const char *capname) const {
        const std::string who = std::string(fn) + ": ";
        if (ndraws < 1 || draw0 < 0 || draw0 > cap || ndraws > cap - draw0)
            return fail(c, DPMM_EINVAL, who + "draw0 >= 0, ndraws >= 1 and draw0 + ndraws <= " + capname + " are needed");
        if (i0 < 0 || (i0 >> 62)) return fail(c, DPMM_EINVAL, who + "i0 out of range");
        if (ld < W) return fail(c, DPMM_EINVAL, who + "ld < " + wname);
        if ((ld >> 40) || draw_stride < 0 || (draw_stride >> 37)) return fail(c, DPMM_EINVAL, who + "ld / draw_stride out of range");
        const bool interleaved = draw_stride >= W && draw_stride <= ld / ndraws;
        if (!interleaved && (unsigned __int128)draw_stride < (unsigned __int128)c->n * (unsigned __int128)ld)
            return fail(c, DPMM_EINVAL, who + "the draws overlap: draw_stride >= n_local * ld (stacked) or " + wname + " <= draw_stride <= ld / ndraws (interleaved) is needed");
        return DPMM_OK;
    }
    // with points (n_local > 0): the state, the pointers and, device variant, their extents
    int ready(dpmm_ctx *c, const char *fn) const {
        const std::string who = std::string(fn) + ": ";
        if (!c->have_points || !c->have_params || !c->dX) return fail(c, DPMM_ESTATE, who + "needs points and parameters");
        if (!out) return fail(c, DPMM_EINVAL, who + "out is null");
        if (!device) return DPMM_OK;
        const uint64_t words = (uint64_t)(ndraws - 1) * (uint64_t)draw_stride + (uint64_t)(c->n - 1) * (uint64_t)ld + (uint64_t)std::min(ld, draw_stride);
        if (int rc = check_device_extent(c, fn, "d_out", out, words * sizeof(float), sizeof(float))) return rc;
        if (comp) if (int rc = check_device_extent(c, fn, "d_comp", comp, (uint64_t)ndraws * (uint64_t)c->n * sizeof(int32_t), sizeof(int32_t))) return rc;
        return DPMM_OK;
    }
    // the draws of a batch for ranges of P_ points: `most` at most (what the call's own scratch per draw allows), host variant 64 MiB of
    // staged draws, one draw at least; the staging block grown to hold them (`who`: the name in its out-of-memory message)
    int size(dpmm_ctx *c, const char *who, int64_t P_, int64_t most) {
        P = P_;
        batch = std::max<int64_t>(1, std::min(ndraws, most));
        if (device) return DPMM_OK;
        batch = std::max<int64_t>(1, std::min<int64_t>(batch, ((int64_t)64 << 20) / ((int64_t)sizeof(float) * P * W)));
        return grow(c, c->d_score_out, (size_t)batch * (size_t)P * (sizeof(float) * (size_t)W + sizeof(int32_t)), who, "staging of the outputs");
    }
    // one range (np points from point p0), batch by batch: launch(j0, nb, dest) -> int or hipError_t
    template <class Launch>
    int range(dpmm_ctx *c, const char *fn, int64_t p0, int64_t np, Launch launch) const {
        const int64_t n = c->n, width = std::min(ld, draw_stride);
        for (int64_t j0 = 0; j0 < ndraws; j0 += batch) {
            const int64_t nb = std::min(batch, ndraws - j0);
            DrawDest d{out + j0 * draw_stride + p0 * ld, ld, draw_stride, comp ? comp + j0 * n + p0 : nullptr, n};
            if (!device) {
                float *st = reinterpret_cast<float *>(c->d_score_out.get());
                d = DrawDest{st, W, np * W, comp ? reinterpret_cast<int32_t *>(st + batch * P * W) : nullptr, np};
            }
            if (int rc = table_result(c, fn, launch(j0, nb, d))) return rc;
            if (device) continue;
            for (int64_t jd = 0; jd < nb; ++jd)
                HIPCHK(c, hipMemcpy2DAsync(out + (j0 + jd) * draw_stride + p0 * ld, sizeof(float) * (size_t)ld, d.out + jd * np * W, sizeof(float) * (size_t)W,
                                           sizeof(float) * (size_t)W, (size_t)np, hipMemcpyDeviceToHost, c->stream));
            if (comp) HIPCHK(c, hipMemcpy2DAsync(comp + j0 * n + p0, sizeof(int32_t) * (size_t)n, d.comp, sizeof(int32_t) * (size_t)np, sizeof(int32_t) * (size_t)np,
                                                 (size_t)nb, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, sync_stream(c, c->stream));      // the staging block is rewritten by the next batch
            if (width > W)
                for (int64_t jd = j0; jd < j0 + nb; ++jd)
                    for (int64_t i = p0; i < p0 + np; ++i) memset(out + jd * draw_stride + i * ld + W, 0, sizeof(float) * (size_t)(width - W));
        }
        return DPMM_OK;
    }
};
}  // extern "C++"

static int score_points(dpmm_ctx *c, const dpmm_score_out *o, bool device, const char *fn) {
    if (!c) return tensor_no_ctx(fn);
    c->miss_counted = false;      // (dpmm_score_missing_counts speaks of THIS call from here on, also where it returns early)
    const std::string who = std::string(fn) + ": ";
    if (!o) return fail(c, DPMM_EINVAL, who + "out is null");
    if (o->m < 0 || o->m > DPMM_SCORE_MAX_TOP) return fail(c, DPMM_EINVAL, who + "m must be in 0.." + std::to_string(DPMM_SCORE_MAX_TOP));
    if (o->m == 0 && (o->top_idx || o->top_prob)) return fail(c, DPMM_EINVAL, who + "top_idx / top_prob given with m = 0");
    if (o->m > 0 && !o->top_idx && !o->top_prob) return fail(c, DPMM_EINVAL, who + "m > 0 needs top_idx or top_prob");
    if (!o->labels && !o->logdens && !o->top_idx && !o->top_prob && !o->probs) return fail(c, DPMM_EINVAL, who + "every output pointer is null");
    if (!c->predictive) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_predictive_* first");
    if (o->m > c->K) return fail(c, DPMM_EINVAL, who + "m exceeds the number of clusters");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0) return DPMM_OK;
    if (!c->have_points || !c->have_params) return fail(c, DPMM_ESTATE, who + "needs points and parameters");
    const size_t K = (size_t)c->K, m = (size_t)o->m;
    OutStage<5> out{{{o->labels, "labels", 8, sizeof(int64_t)}, {o->logdens, "logdens", 4, sizeof(float)}, {o->top_idx, "top_idx", 8, sizeof(int64_t) * m},
                     {o->top_prob, "top_prob", 4, sizeof(float) * m}, {o->probs, "probs", 4, sizeof(float) * K}}, device};
    if (int rc = out.check(c, fn, (uint64_t)c->n)) return rc;
    TableWalk w;
    if (int rc = walk_open(c, fn, WALK_MISS_OPTION, &w)) return rc;
    if (int rc = out.open(c, w.P)) return rc;
    if (int rc = walk_ranges(c, w, c->n, fn, [&](int64_t p0, int64_t np, int64_t) {
            ScoreArgs a{};
            a.table = c->d_score_table; a.stride = w.P; a.rstep = w.rstep; a.n = np; a.K = c->K; a.m = o->m;
            a.labels = out.at<int64_t>(0, p0); a.logdens = out.at<float>(1, p0);
            a.top_idx = out.at<int64_t>(2, p0); a.top_prob = out.at<float>(3, p0); a.probs = out.at<float>(4, p0);
            hipError_t e = launch_score_finish(a, c->stream);
            if (e == hipSuccess && !device) e = out.flush(c, p0, (size_t)np);
            return e;
        })) return rc;
    return device ? table_result(c, fn, sync_stream(c, c->stream)) : DPMM_OK;
}

int dpmm_score_points(dpmm_ctx *c, const dpmm_score_out *out) { return score_points(c, out, false, "dpmm_score_points"); }
int dpmm_score_points_device(dpmm_ctx *c, const dpmm_score_out *out) { return score_points(c, out, true, "dpmm_score_points_device"); }

int dpmm_score_missing_counts(dpmm_ctx *c, int64_t out[2]) {
    static const char *fn = "dpmm_score_missing_counts";
    if (!c) return tensor_no_ctx(fn);
    if (!out) return fail(c, DPMM_EINVAL, std::string(fn) + ": out is null");
    out[0] = out[1] = 0;
    if (!c->miss_counted) return DPMM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_stream(c, c->stream));
    unsigned long long h[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpy(h, c->d_miss_cnt, sizeof(h), hipMemcpyDeviceToHost));
    out[0] = (int64_t)h[1]; out[1] = (int64_t)h[2];
    return DPMM_OK;
}

// ---- include/dpmm_hip_typicality.h: label, q = |R_k (x - m_k)|^2 of the point's own cluster and its tail, range by range (typicality.hip) ----
// The scratch of one range of P points (class words, q) and the three counters; the parameter copies of missing.hip are those in force.
static int typ_begin(dpmm_ctx *c, int64_t P, const char *fn) {
    if (int rc = grow(c, c->d_typ_cls, sizeof(int32_t) * (size_t)P, "dpmm_score_points", "class words of the typicality pass")) return rc;
    if (int rc = grow(c, c->d_typ_q, sizeof(float) * (size_t)P, "dpmm_score_points", "squared distances of the typicality pass")) return rc;
    if (int rc = grow(c, c->d_typ_cnt, 3 * sizeof(unsigned long long), "dpmm_score_points", "counters of the typicality pass")) return rc;
    return miss_params(c, fn);
}

// One range of the table (np points from point p0, rows P floats apart), just evaluated (and patched) on the ctx stream.  labels, q, tail:
// device memory of np entries or null; q == null: the ctx's scratch.  The counters are added to.  gaps: the walk's missing-feature pass has
// just listed this range's points with gaps, and q and tail of those are marginalised (DPMM_OPT_TYPICALITY_GAPS).
static int typ_range(dpmm_ctx *c, int64_t P, int64_t p0, int64_t np, int64_t *labels, float *q, float *tail, const char *fn, bool gaps = false) {
    TypicalityArgs a = niw_range_args<TypicalityArgs>(c, P, p0, np);
    a.cls = c->d_typ_cls; a.labels = labels; a.q = q ? q : c->d_typ_q.get(); a.tail = tail; a.cnt = c->d_typ_cnt;
    if (gaps) { a.list = c->d_miss_list; a.list_cnt = c->d_miss_cnt; }
    return table_result(c, fn, launch_typicality_range(a, 32 * c->cus, c->stream));
}

// The device copies explain.hip and explain_group.hip read beside miss_params' -- the row-major factors Rr and the diagonals a of R'R -- are
// those of the predictive set in force afterwards.  Called behind miss_params (typ_begin), which has checked the prior and the parameters.
static int explain_params(dpmm_ctx *c) {
    if (c->exp_gen == c->pred_gen) return DPMM_OK;
    const size_t K = (size_t)c->K, D = (size_t)c->D, Dp = (size_t)miss_pitch(c->D);
    if (int rc = grow(c, c->d_exp_rr, sizeof(float) * K * D * Dp, "dpmm_explain_points", "row-major factors of the explain pass")) return rc;
    if (int rc = grow(c, c->d_exp_a, sizeof(float) * K * Dp, "dpmm_explain_points", "diagonals of the explain pass")) return rc;
    const ParLayout L = par_layout(c, c->miss_slots);
    const float *Rpk = reinterpret_cast<const float *>(c->d_par + (L.mat - L.cst));      // (as miss_params)
    HIPCHK(c, launch_explain_params(Rpk, 3 * (int64_t)(D * (D + 1) / 2), c->d_exp_rr, c->d_exp_a, c->K, c->D, c->stream));
    c->exp_gen = c->pred_gen;
    return DPMM_OK;
}

// ---- what typicality_points, explain_points and explain_groups_points share around their walk
extern "C++" {
// What the three refuse first, in this order: no ctx, no out, the prior (`what`: the name in the message of what the call computes), own(0),
// every output pointer null (rows: a row output of the call's own is given), own(1), no predictive set, own(2); then skipped and incomplete
// zeroed and, with points, the state.  own(at) -> int: the call's own refusals at that place.  The caller returns behind it where n_local = 0.
template <class Out, class Own>
static int typ_front(dpmm_ctx *c, const char *fn, const Out *o, const char *what, bool rows, Own own) {
    if (!c) return tensor_no_ctx(fn);
    c->miss_counted = false;      // (as score_points)
    const std::string who = std::string(fn) + ": ";
    if (!o) return fail(c, DPMM_EINVAL, who + "out is null");
    if (c->prior != DPMM_PRIOR_NIW)
        return fail(c, DPMM_EINVAL, who + "the " + what + " is that of the NIW prior's Student-t predictive; the Multinomial predictive has no closed-form tail");
    if (int rc = own(0)) return rc;
    if (!o->labels && !o->mahalanobis && !o->tail && !o->skipped && !o->incomplete && !rows) return fail(c, DPMM_EINVAL, who + "every output pointer is null");
    if (int rc = own(1)) return rc;
    if (!c->predictive) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_predictive_niw first");
    if (int rc = own(2)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (o->skipped) o->skipped[0] = 0;
    if (o->incomplete) o->incomplete[0] = 0;
    if (c->n > 0 && (!c->have_points || !c->have_params || !c->dX)) return fail(c, DPMM_ESTATE, who + "needs points and parameters");
    return DPMM_OK;
}
// the range typ_range has just classified as the kernels of the row outputs take it (ExplainArgs, ExplainGroupArgs): the copies and the means
// the typicality pass has read, the row-major factors, the class words
template <class Args>
static Args explain_range_args(dpmm_ctx *c, int64_t P, int64_t p0, int64_t np) {
    const TypicalityArgs t = niw_range_args<TypicalityArgs>(c, P, p0, np);
    Args a{};
    a.n = t.n; a.K = t.K; a.D = t.D; a.X = t.X; a.ldx = t.ldx; a.Rt = t.Rt; a.mu = t.mu; a.mu_step = t.mu_step; a.cst = t.cst;
    a.Rr = c->d_exp_rr; a.cls = c->d_typ_cls;
    return a;
}
}  // extern "C++"
// behind the extents: the walk opened, the scratch of the pass, with row outputs the copies explain.hip reads, the three counters cleared
static int typ_open(dpmm_ctx *c, const char *fn, TableWalk *w, bool rows) {
    if (int rc = walk_open(c, fn, WALK_MISS_OPTION, w)) return rc;
    if (int rc = typ_begin(c, w->P, fn)) return rc;
    if (rows) if (int rc = explain_params(c)) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_typ_cnt, 0, 3 * sizeof(unsigned long long), c->stream));
    return DPMM_OK;
}
// behind the last range: the wait for the ctx stream, then the counters into skipped[0] and incomplete[0] (null: not asked for)
static int typ_counters(dpmm_ctx *c, int64_t *skipped, int64_t *incomplete) {
    HIPCHK(c, sync_stream(c, c->stream));
    unsigned long long h[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpy(h, c->d_typ_cnt, sizeof(h), hipMemcpyDeviceToHost));
    if (skipped) skipped[0] = (int64_t)h[0];
    if (incomplete) incomplete[0] = (int64_t)(h[1] - h[2]);      // (h[2]: scored with gaps, 0 where no call passes the list)
    return DPMM_OK;
}

static int typicality_points(dpmm_ctx *c, const dpmm_typicality_out *o, bool device, const char *fn) {
    if (int rc = typ_front(c, fn, o, "tail", false, [](int) { return DPMM_OK; })) return rc;
    if (c->n == 0) return DPMM_OK;
    OutStage<3> out{{{o->labels, "labels", 8, sizeof(int64_t)}, {o->mahalanobis, "mahalanobis", 4, sizeof(float)}, {o->tail, "tail", 4, sizeof(float)}}, device};
    if (int rc = out.check(c, fn, (uint64_t)c->n)) return rc;
    TableWalk w;
    if (int rc = typ_open(c, fn, &w, false)) return rc;
    if (int rc = out.open(c, w.P)) return rc;
    const bool gaps = w.miss && c->opt_typ_gaps != 0;      // (without a list nothing new runs)
    if (int rc = walk_ranges(c, w, c->n, fn, [&](int64_t p0, int64_t np, int64_t) -> int {
            if (int rc = typ_range(c, w.P, p0, np, out.at<int64_t>(0, p0), out.at<float>(1, p0), out.at<float>(2, p0), fn, gaps)) return rc;
            return device ? DPMM_OK : table_result(c, fn, out.flush(c, p0, (size_t)np));
        })) return rc;
    return typ_counters(c, o->skipped, o->incomplete);
}

int dpmm_typicality_points(dpmm_ctx *c, const dpmm_typicality_out *out) { return typicality_points(c, out, false, "dpmm_typicality_points"); }
int dpmm_typicality_points_device(dpmm_ctx *c, const dpmm_typicality_out *out) { return typicality_points(c, out, true, "dpmm_typicality_points_device"); }

// ---- include/dpmm_hip_explain.h: behind the typicality pass of every range, the per-feature residuals, z-scores and tails (explain.hip) ----
static int explain_points(dpmm_ctx *c, const dpmm_explain_out *o, bool device, const char *fn) {
    const std::string who = std::string(fn) + ": ";
    const bool rows = o && (o->residual || o->zscore || o->feature_tail || o->features);
    int64_t width = 0;
    if (int rc = typ_front(c, fn, o, "explanation", rows, [&](int at) -> int {
            if (at == 0) {
                const int cap = std::min(c->D, DPMM_EXPLAIN_MAX_TOP);
                if (o->top < 0 || o->top > cap) return fail(c, DPMM_EINVAL, who + "top must be in 0.." + std::to_string(cap));
                if (o->top == 0 && o->features) return fail(c, DPMM_EINVAL, who + "features given with top = 0");
                width = o->top ? o->top : c->D;
            }
            if (at == 1 && rows) {
                if (o->ld < width) return fail(c, DPMM_EINVAL, who + "ld < " + (o->top ? "top" : "D"));
                if (o->ld >> 31) return fail(c, DPMM_EINVAL, who + "ld out of range (below 2^31)");
            }
            return DPMM_OK;
        })) return rc;
    if (c->n == 0) return DPMM_OK;
    const uint64_t n = (uint64_t)c->n, ld = rows ? (uint64_t)o->ld : 0;
    if (ld && n > (UINT64_MAX / sizeof(int64_t)) / ld) return fail(c, DPMM_EINVAL, who + "n_local * ld out of range");      // (the extents below cannot wrap)
    // the rows: in the caller's memory ld entries apart, the words behind `width` left as they are; staged (host variant) dense, `width` apart
    // (`1, false, true`: one row a point, an output, keep)
    const size_t rb = 4 * (size_t)width, pb = 4 * (size_t)ld;      // (4-byte entries all)
    OutStage<7> out{{{o->labels, "labels", 8, sizeof(int64_t)}, {o->mahalanobis, "mahalanobis", 4, sizeof(float)}, {o->tail, "tail", 4, sizeof(float)},
                     {o->residual, "residual", 4, rb, pb, 1, false, true}, {o->zscore, "zscore", 4, rb, pb, 1, false, true},
                     {o->feature_tail, "feature_tail", 4, rb, pb, 1, false, true}, {o->features, "features", 4, rb, pb, 1, false, true}}, device};
    if (int rc = out.check(c, fn, n)) return rc;
    TableWalk w;
    if (int rc = typ_open(c, fn, &w, rows)) return rc;
    if (int rc = out.open(c, w.P)) return rc;
    const bool gaps = w.miss && c->opt_typ_gaps != 0;      // (without a list nothing new runs)
    if (int rc = walk_ranges(c, w, c->n, fn, [&](int64_t p0, int64_t np, int64_t) -> int {
            if (int rc = typ_range(c, w.P, p0, np, out.at<int64_t>(0, p0), out.at<float>(1, p0), out.at<float>(2, p0), fn, gaps)) return rc;
            if (rows) {
                ExplainArgs a = explain_range_args<ExplainArgs>(c, w.P, p0, np);
                a.a = c->d_exp_a;
                a.residual = out.at<float>(3, p0); a.zscore = out.at<float>(4, p0); a.feature_tail = out.at<float>(5, p0); a.features = out.at<int32_t>(6, p0);
                a.top = o->top; a.ld = device ? (int64_t)ld : width;
                if (gaps) { a.list = c->d_miss_list; a.list_cnt = c->d_miss_cnt; }
                if (int rc = table_result(c, fn, launch_explain_range(a, 32 * c->cus, c->stream))) return rc;
                if (gaps) if (int rc = table_result(c, fn, launch_explain_gap_range(a, 32 * c->cus, c->stream))) return rc;
            }
            return device ? DPMM_OK : table_result(c, fn, out.flush(c, p0, (size_t)np));
        })) return rc;
    return typ_counters(c, o->skipped, o->incomplete);
}

int dpmm_explain_points(dpmm_ctx *c, const dpmm_explain_out *out) { return explain_points(c, out, false, "dpmm_explain_points"); }
int dpmm_explain_points_device(dpmm_ctx *c, const dpmm_explain_out *out) { return explain_points(c, out, true, "dpmm_explain_points_device"); }

// ---- include/dpmm_hip_explain_groups.h: behind the typicality pass of every range, q_G and its tail for every group (explain_group.hip) ----
static_assert(DPMM_EXPLAIN_MAX_GROUPS == EXPLAIN_MAX_GROUPS, "header / kernel limits out of sync");
int dpmm_set_explain_groups(dpmm_ctx *c, int32_t G, const int64_t *offsets, const int32_t *features, const double *W) {
    static const char *fn = "dpmm_set_explain_groups";
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, who + "the explanation is that of the NIW prior's Student-t predictive; the Multinomial predictive has no closed-form tail");
    if (G < 1 || G > DPMM_EXPLAIN_MAX_GROUPS) return fail(c, DPMM_EINVAL, who + "G must be in 1.." + std::to_string(DPMM_EXPLAIN_MAX_GROUPS));
    if (!offsets) return fail(c, DPMM_EINVAL, who + "offsets is null");
    if (!features) return fail(c, DPMM_EINVAL, who + "features is null");
    if (!W) return fail(c, DPMM_EINVAL, who + "W is null");
    if (!c->predictive) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_predictive_niw first");
    const int64_t D = c->D;
    if (offsets[0] != 0) return fail(c, DPMM_EINVAL, who + "offsets[0] must be 0");
    for (int j = 0; j < G; ++j)
        if (offsets[j + 1] <= offsets[j] || offsets[j + 1] > D)
            return fail(c, DPMM_EINVAL, who + "offsets must increase strictly (no empty group) and end at D at most, group " + std::to_string(j));
    std::vector<char> seen((size_t)D, 0);
    for (int j = 0; j < G; ++j)
        for (int64_t e = offsets[j]; e < offsets[j + 1]; ++e) {
            const int64_t f = features[e];
            if (f < 0 || f >= D) return fail(c, DPMM_EINVAL, who + "features out of 0..D-1 in group " + std::to_string(j));
            if (e > offsets[j] && f <= features[e - 1]) return fail(c, DPMM_EINVAL, who + "features must increase strictly inside group " + std::to_string(j));
            if (seen[(size_t)f]) return fail(c, DPMM_EINVAL, who + "features: feature " + std::to_string(f) + " is in two groups");
            seen[(size_t)f] = 1;
        }
    // the images: descriptors, first words, and per cluster and group the columns of W padded to explain_group_pitch(s) rows, rounded once
    const size_t K = (size_t)c->K, total = (size_t)offsets[G];
    std::vector<int32_t> desc((size_t)G + 1 + total);
    std::vector<int64_t> gw((size_t)G);
    size_t wstep = 0, tri = 0;
    for (int j = 0; j < G; ++j) {
        const size_t s = (size_t)(offsets[j + 1] - offsets[j]);
        desc[(size_t)j] = (int32_t)offsets[j];
        gw[(size_t)j] = (int64_t)wstep;
        wstep += s * (size_t)explain_group_pitch((int)s);
        tri += s * (s + 1) / 2;
    }
    desc[(size_t)G] = (int32_t)total;
    for (size_t e = 0; e < total; ++e) desc[(size_t)G + 1 + e] = features[e];
    std::vector<float> img(K * wstep, 0.f);
    for (size_t k = 0; k < K; ++k) {
        const double *src = W + k * tri;
        for (int j = 0; j < G; ++j) {
            const size_t s = (size_t)(offsets[j + 1] - offsets[j]), sp = (size_t)explain_group_pitch((int)s);
            float *dst = img.data() + k * wstep + (size_t)gw[(size_t)j];
            for (size_t r = 0; r < s; ++r)
                for (size_t cc = 0; cc <= r; ++cc) {
                    const double w = *src++;
                    if (!std::isfinite(w) || !std::isfinite((float)w)) return fail(c, DPMM_EINVAL, who + "W holds a value that is not finite (in Float32), cluster " + std::to_string(k) + " group " + std::to_string(j));
                    dst[cc * sp + r] = (float)w;
                }
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    c->exg_gen = 0;      // (a failure below leaves no tables in force)
    if (int rc = grow(c, c->d_exg_w, sizeof(float) * img.size(), fn, "group tables")) return rc;
    if (int rc = grow(c, c->d_exg_desc, sizeof(int32_t) * desc.size(), fn, "group descriptors")) return rc;
    if (int rc = grow(c, c->d_exg_gw, sizeof(int64_t) * gw.size(), fn, "group descriptors")) return rc;
    HIPCHK(c, sync_stream(c, c->stream));
    HIPCHK(c, hipMemcpy(c->d_exg_w, img.data(), sizeof(float) * img.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_exg_desc, desc.data(), sizeof(int32_t) * desc.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_exg_gw, gw.data(), sizeof(int64_t) * gw.size(), hipMemcpyHostToDevice));
    c->exg_G = G; c->exg_wstep = (int64_t)wstep;
    c->exg_gen = c->pred_gen;
    return DPMM_OK;
}

static int explain_groups_points(dpmm_ctx *c, const dpmm_explain_groups_out *o, bool device, const char *fn) {
    const std::string who = std::string(fn) + ": ";
    const bool rows = o && (o->group_mahalanobis || o->group_tail);
    if (int rc = typ_front(c, fn, o, "explanation", rows, [&](int at) -> int {
            if (at != 2) return DPMM_OK;
            if (c->exg_gen == 0 || c->exg_gen != c->pred_gen) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_explain_groups for the predictive parameters in force");
            if (rows && o->ld < c->exg_G) return fail(c, DPMM_EINVAL, who + "ld < G");
            if (rows && (o->ld >> 31)) return fail(c, DPMM_EINVAL, who + "ld out of range (below 2^31)");
            return DPMM_OK;
        })) return rc;
    if (c->n == 0) return DPMM_OK;
    const int64_t width = c->exg_G;
    const uint64_t n = (uint64_t)c->n, ld = rows ? (uint64_t)o->ld : 0;
    if (ld && n > (UINT64_MAX / sizeof(int64_t)) / ld) return fail(c, DPMM_EINVAL, who + "n_local * ld out of range");      // (the extents below cannot wrap)
    // the rows: as explain_points -- ld entries apart, the words behind the G entries left as they are; staged (host variant) dense
    const size_t rb = sizeof(float) * (size_t)width, pb = sizeof(float) * (size_t)ld;
    OutStage<5> out{{{o->labels, "labels", 8, sizeof(int64_t)}, {o->mahalanobis, "mahalanobis", 4, sizeof(float)}, {o->tail, "tail", 4, sizeof(float)},
                     {o->group_mahalanobis, "group_mahalanobis", 4, rb, pb, 1, false, true}, {o->group_tail, "group_tail", 4, rb, pb, 1, false, true}}, device};
    if (int rc = out.check(c, fn, n)) return rc;
    TableWalk w;
    if (int rc = typ_open(c, fn, &w, rows)) return rc;      // (the row-major factors of explain.hip)
    if (int rc = out.open(c, w.P)) return rc;
    if (int rc = walk_ranges(c, w, c->n, fn, [&](int64_t p0, int64_t np, int64_t) -> int {
            if (int rc = typ_range(c, w.P, p0, np, out.at<int64_t>(0, p0), out.at<float>(1, p0), out.at<float>(2, p0), fn)) return rc;
            if (rows) {
                ExplainGroupArgs a = explain_range_args<ExplainGroupArgs>(c, w.P, p0, np);
                a.G = c->exg_G;
                a.goff = c->d_exg_desc; a.gfeat = c->d_exg_desc + (c->exg_G + 1); a.gw = c->d_exg_gw; a.W = c->d_exg_w; a.wstep = c->exg_wstep;
                a.group_q = out.at<float>(3, p0); a.group_tail = out.at<float>(4, p0); a.ld = device ? (int64_t)ld : width;
                if (int rc = table_result(c, fn, launch_explain_group_range(a, 32 * c->cus, c->stream))) return rc;
            }
            return device ? DPMM_OK : table_result(c, fn, out.flush(c, p0, (size_t)np));
        })) return rc;
    return typ_counters(c, o->skipped, o->incomplete);
}

int dpmm_explain_groups_points(dpmm_ctx *c, const dpmm_explain_groups_out *out) { return explain_groups_points(c, out, false, "dpmm_explain_groups_points"); }
int dpmm_explain_groups_points_device(dpmm_ctx *c, const dpmm_explain_groups_out *out) { return explain_groups_points(c, out, true, "dpmm_explain_groups_points_device"); }

static int impute_points(dpmm_ctx *c, float *out, int64_t ld, bool device, const char *fn) {
    if (!c) return tensor_no_ctx(fn);
    c->miss_counted = false;      // (as score_points)
    const std::string who = std::string(fn) + ": ";
    if (c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, who + "the Multinomial prior has no missing features");
    if (!c->predictive) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_predictive_niw first");
    if (ld < c->D) return fail(c, DPMM_EINVAL, who + "ld < D");
    if (ld >> 40) return fail(c, DPMM_EINVAL, who + "ld out of range");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0) return DPMM_OK;
    if (!c->have_points || !c->have_params || !c->dX) return fail(c, DPMM_ESTATE, who + "needs points and parameters");
    if (!out) return fail(c, DPMM_EINVAL, who + "out is null");
    // the rows: in the caller's device memory ld floats apart; staged (host variant) dense, D apart
    OutStage<1> st{{{out, "d_out", 4, sizeof(float) * (size_t)c->D, sizeof(float) * (size_t)ld}}, device};
    if (int rc = st.check(c, fn, (uint64_t)c->n)) return rc;
    TableWalk w;
    if (int rc = walk_open(c, fn, WALK_MISS_ALWAYS, &w)) return rc;
    w.miss = false;      // the consumer patches: the rows the imputation is written behind are copied first
    if (int rc = st.open(c, w.P)) return rc;
    if (int rc = walk_ranges(c, w, c->n, fn, [&](int64_t p0, int64_t np, int64_t) -> int {
            float *rows = st.at<float>(0, p0);
            const int64_t ldr = device ? ld : c->D;
            HIPCHK(c, launch_points_readback(rows, ldr, c->dX + p0 * c->ldx, c->ldx, nullptr, 0, np, c->D, c->stream));
            if (int rc = miss_range(c, w.P, p0, np, rows, ldr, fn)) return rc;
            return device ? DPMM_OK : table_result(c, fn, st.flush(c, p0, (size_t)np));
        })) return rc;
    HIPCHK(c, sync_stream(c, c->stream));
    return DPMM_OK;
}

int dpmm_impute_points(dpmm_ctx *c, float *out, int64_t ld) { return impute_points(c, out, ld, false, "dpmm_impute_points"); }
int dpmm_impute_points_device(dpmm_ctx *c, float *d_out, int64_t ld) { return impute_points(c, d_out, ld, true, "dpmm_impute_points_device"); }

// ---- include/dpmm_hip_impute.h: draws of the missing features.  Per range: the table once, list and patch, then the draws (DrawBatch).
static int impute_draw_points(dpmm_ctx *c, float *out, int64_t ld, int64_t draw_stride, int32_t *comp, uint64_t seed, int64_t i0, int64_t draw0,
                              int64_t ndraws, bool device, const char *fn) {
    if (!c) return tensor_no_ctx(fn);
    c->miss_counted = false;      // (as score_points)
    const std::string who = std::string(fn) + ": ";
    if (c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, who + "the Multinomial prior has no missing features");
    if (!c->predictive) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_predictive_niw first");
    DrawBatch b{out, ld, draw_stride, comp, ndraws, device, c->D, "D"};
    if (int rc = b.check(c, fn, i0, draw0, DPMM_IMPUTE_MAX_DRAWS, "DPMM_IMPUTE_MAX_DRAWS")) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0) return DPMM_OK;
    if (int rc = b.ready(c, fn)) return rc;
    TableWalk tw;
    if (int rc = walk_open(c, fn, WALK_MISS_ALWAYS, &tw)) return rc;
    if (int rc = b.size(c, "dpmm_score_points", tw.P, ndraws)) return rc;
    if (int rc = walk_ranges(c, tw, c->n, fn, [&](int64_t p0, int64_t np, int64_t) -> int {
            MissArgs a = niw_range_args<MissArgs>(c, tw.P, p0, np);
            a.list = c->d_miss_list; a.cnt = c->d_miss_cnt;      // the list the walk's pass has just made of this range
            return b.range(c, fn, p0, np, [&](int64_t j0, int64_t nb, const DrawDest &d) {
                MissDraw w{};
                w.seed = seed; w.i0 = i0 + p0; w.draw0 = draw0 + j0; w.ndraws = (int)nb;
                w.out = d.out; w.ld = d.ld; w.draw_stride = d.draw_stride; w.comp = d.comp; w.comp_stride = d.comp_stride;
                return launch_miss_draw(a, w, 8 * c->cus, c->stream);
            });
        })) return rc;
    HIPCHK(c, sync_stream(c, c->stream));
    return DPMM_OK;
}

int dpmm_impute_draw_points(dpmm_ctx *c, float *out, int64_t ld, int64_t draw_stride, int32_t *comp, uint64_t seed, int64_t i0, int64_t draw0, int64_t ndraws) {
    return impute_draw_points(c, out, ld, draw_stride, comp, seed, i0, draw0, ndraws, false, "dpmm_impute_draw_points");
}
int dpmm_impute_draw_points_device(dpmm_ctx *c, float *d_out, int64_t ld, int64_t draw_stride, int32_t *d_comp, uint64_t seed, int64_t i0, int64_t draw0,
                                   int64_t ndraws) {
    return impute_draw_points(c, d_out, ld, draw_stride, d_comp, seed, i0, draw0, ndraws, true, "dpmm_impute_draw_points_device");
}

// ---- include/dpmm_hip_regress.h: the mixture of the clusters' conditional means and its spread, range by range (regress.hip) -------------
int dpmm_set_regression(dpmm_ctx *c, int Dt, const double *B, const double *cc, const double *V, const double *h) {
    static const char *fn = "dpmm_set_regression";
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, who + "the regression is that of the NIW prior's Student-t predictive");
    if (Dt < 1 || Dt > DPMM_REGRESS_MAX_TARGETS) return fail(c, DPMM_EINVAL, who + "D_t must be in 1.." + std::to_string(DPMM_REGRESS_MAX_TARGETS));
    if (!B || !cc || !V || !h) return fail(c, DPMM_EINVAL, who + "null table");
    if (!c->predictive || c->h_miss_cst.size() != (size_t)c->K * MISS_CST) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_predictive_niw first");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t K = (size_t)c->K, D = (size_t)c->D, Tp = (size_t)regress_pitch(Dt);
    c->reg_gen = 0;      // (a failure below leaves no tables in force)
    c->reg_factor = false;      // (the factor's image holds a copy of the matrices that are about to be replaced)
    c->reg_lev_gen = 0;         // (the levels' z belong to the tables that are about to be replaced)
    if (int rc = grow(c, c->d_reg_bt, sizeof(float) * K * D * Tp, fn, "regression matrices")) return rc;
    if (int rc = grow(c, c->d_reg_c, sizeof(float) * K * Tp, fn, "regression offsets")) return rc;
    if (int rc = grow(c, c->d_reg_v, sizeof(float) * K * Tp, fn, "regression variances")) return rc;
    if (int rc = grow(c, c->d_reg_hd, sizeof(double) * 2 * K, fn, "regression constants")) return rc;
    // each value rounded to Float32 once; B transposed to [K][D][Tp], zeros in the pad
    std::vector<float> bt(K * D * Tp, 0.f), cv(K * Tp, 0.f), vv(K * Tp, 0.f);
    std::vector<double> hd(2 * K);
    bool no_var = false;
    for (size_t k = 0; k < K; ++k) {
        for (size_t d = 0; d < (size_t)Dt; ++d) {
            for (size_t e = 0; e < D; ++e) bt[(k * D + e) * Tp + d] = (float)B[(k * (size_t)Dt + d) * D + e];
            cv[k * Tp + d] = (float)cc[k * (size_t)Dt + d];
            vv[k * Tp + d] = (float)V[k * (size_t)Dt + d];
        }
        hd[2 * k] = h[k];
        hd[2 * k + 1] = c->h_miss_cst[k * MISS_CST];      // df_k, the Float32 value the table kernel reads, widened
        if (!(hd[2 * k + 1] + (double)D > 2.0)) no_var = true;
    }
    HIPCHK(c, sync_stream(c, c->stream));
    HIPCHK(c, hipMemcpy(c->d_reg_bt, bt.data(), sizeof(float) * bt.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_reg_c, cv.data(), sizeof(float) * cv.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_reg_v, vv.data(), sizeof(float) * vv.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_reg_hd, hd.data(), sizeof(double) * hd.size(), hipMemcpyHostToDevice));
    c->reg_Dt = Dt;
    c->reg_no_var = no_var;
    c->reg_gen = c->pred_gen;
    return DPMM_OK;
}

static int regress_points(dpmm_ctx *c, float *mean, float *sd, int64_t ld, int64_t *labels, int64_t *skipped, bool device, const char *fn) {
    if (int rc = regress_front(c, fn, REGRESS_TABLES)) return rc;
    const std::string who = std::string(fn) + ": ";
    const int64_t Dt = c->reg_Dt;
    if (ld < Dt) return fail(c, DPMM_EINVAL, who + "ld < D_t");
    if (ld >> 40) return fail(c, DPMM_EINVAL, who + "ld out of range");
    if (sd && c->reg_no_var) return fail(c, DPMM_EINVAL, who + "a cluster has df + D <= 2: its conditional law has no variance");
    HIPCHK(c, hipSetDevice(c->device));
    if (skipped) skipped[0] = 0;
    if (c->n == 0) return DPMM_OK;
    if (!c->have_points || !c->have_params || !c->dX) return fail(c, DPMM_ESTATE, who + "needs points and parameters");
    if (!mean) return fail(c, DPMM_EINVAL, who + "mean is null");
    // the rows: in the caller's device memory ld floats apart; staged (host variant) dense, D_t apart
    const size_t row = sizeof(float) * (size_t)Dt, pitch = sizeof(float) * (size_t)ld;
    OutStage<3> out{{{mean, "d_mean", 4, row, pitch}, {sd, "d_std", 4, row, pitch}, {labels, "d_labels", 8, sizeof(int64_t)}}, device};
    if (int rc = out.check(c, fn, (uint64_t)c->n)) return rc;
    TableWalk w;
    if (int rc = walk_open(c, fn, WALK_MISS_NEVER, &w)) return rc;
    if (int rc = skip_open(c, c->d_reg_skip, w.P, fn, "counts of the regression pass")) return rc;
    if (int rc = out.open(c, w.P)) return rc;
    if (int rc = walk_ranges(c, w, c->n, fn, [&](int64_t p0, int64_t np, int64_t) {
            RegressArgs a{};
            a.t = regress_tile(c, w.P, p0, np, out.at<int64_t>(2, p0), c->d_reg_skip);
            a.Bt = c->d_reg_bt; a.V = c->d_reg_v;
            a.mean = out.at<float>(0, p0); a.std = out.at<float>(1, p0); a.ld = device ? ld : Dt;
            hipError_t e = launch_regress_range(a, c->stream);
            if (e == hipSuccess && !device) e = out.flush(c, p0, (size_t)np);
            return e;
        })) return rc;
    return skip_close(c, c->d_reg_skip, w.P, skipped);
}

int dpmm_regress_points(dpmm_ctx *c, float *mean, float *std, int64_t ld, int64_t *labels, int64_t *skipped) {
    return regress_points(c, mean, std, ld, labels, skipped, false, "dpmm_regress_points");
}
int dpmm_regress_points_device(dpmm_ctx *c, float *d_mean, float *d_std, int64_t ld, int64_t *d_labels, int64_t *skipped) {
    return regress_points(c, d_mean, d_std, ld, d_labels, skipped, true, "dpmm_regress_points_device");
}

// ---- include/dpmm_hip_regress_draw.h: draws of the targets, range by range (regress_draw.hip) -------------------------------------------
int dpmm_set_regression_factor(dpmm_ctx *c, const double *W) {
    static const char *fn = "dpmm_set_regression_factor";
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, who + "the regression is that of the NIW prior's Student-t predictive");
    if (!W) return fail(c, DPMM_EINVAL, who + "null table");
    if (!c->predictive || c->reg_gen == 0 || c->reg_gen != c->pred_gen) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_regression for the predictive parameters in force");
    const size_t K = (size_t)c->K, D = (size_t)c->D, Dt = (size_t)c->reg_Dt, Tp = (size_t)regress_pitch(c->reg_Dt), R = D + Dt;
    if (R > 256) return fail(c, DPMM_EINVAL, who + "D_o + D_t > 256");
    HIPCHK(c, hipSetDevice(c->device));
    c->reg_factor = false;      // (a failure below leaves no factor in force)
    if (int rc = grow(c, c->d_reg_bw, sizeof(float) * K * R * Tp, fn, "regression matrices and factors")) return rc;
    // each value rounded to Float32 once; W transposed to rows [D, D + D_t) of cluster k's image, zeros below the diagonal and in the pad
    std::vector<float> wt(K * Dt * Tp, 0.f);
    for (size_t k = 0; k < K; ++k)
        for (size_t d = 0; d < Dt; ++d)
            for (size_t a = d; a < Dt; ++a) wt[(k * Dt + a) * Tp + d] = (float)W[(k * Dt + d) * Dt + a];
    HIPCHK(c, sync_stream(c, c->stream));
    HIPCHK(c, hipMemcpy2D(c->d_reg_bw, sizeof(float) * R * Tp, c->d_reg_bt, sizeof(float) * D * Tp, sizeof(float) * D * Tp, K, hipMemcpyDeviceToDevice));
    HIPCHK(c, hipMemcpy2D(c->d_reg_bw + D * Tp, sizeof(float) * R * Tp, wt.data(), sizeof(float) * Dt * Tp, sizeof(float) * Dt * Tp, K, hipMemcpyHostToDevice));
    c->reg_factor = true;
    return DPMM_OK;
}

// Per range: the table once, then the draws (DrawBatch)
static int regress_draw_points(dpmm_ctx *c, float *out, int64_t ld, int64_t draw_stride, int32_t *comp, uint64_t seed, int64_t i0, int64_t draw0,
                               int64_t ndraws, int64_t *skipped, bool device, const char *fn) {
    if (int rc = regress_front(c, fn, REGRESS_FACTOR)) return rc;
    DrawBatch b{out, ld, draw_stride, comp, ndraws, device, c->reg_Dt, "D_t"};
    if (int rc = b.check(c, fn, i0, draw0, DPMM_REGRESS_MAX_DRAWS, "DPMM_REGRESS_MAX_DRAWS")) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (skipped) skipped[0] = 0;
    if (c->n == 0) return DPMM_OK;
    if (int rc = b.ready(c, fn)) return rc;
    TableWalk tw;
    if (int rc = walk_open(c, fn, WALK_MISS_NEVER, &tw)) return rc;
    const int64_t P = tw.P;
    if (int rc = skip_open(c, c->d_reg_skip, P, fn, "counts of the regression pass")) return rc;
    if (int rc = b.size(c, fn, P, ((int64_t)16 << 20) / (8 * P))) return rc;      // 16 MiB of components and scales at most
    if (int rc = grow(c, c->d_reg_kc, sizeof(int32_t) * (size_t)b.batch * (size_t)P, fn, "components of a batch of draws")) return rc;
    if (int rc = grow(c, c->d_reg_sc, sizeof(float) * (size_t)b.batch * (size_t)P, fn, "scales of a batch of draws")) return rc;
    if (int rc = walk_ranges(c, tw, c->n, fn, [&](int64_t p0, int64_t np, int64_t) -> int {
            RegressDrawArgs a{};
            a.kc = c->d_reg_kc; a.sc = c->d_reg_sc; a.Bw = c->d_reg_bw;
            a.seed = seed; a.i0 = i0 + p0;
            return b.range(c, fn, p0, np, [&](int64_t j0, int64_t nb, const DrawDest &d) {
                a.t = regress_tile(c, P, p0, np, nullptr, j0 == 0 ? c->d_reg_skip.get() : nullptr);      // a point is counted once per call
                a.draw0 = draw0 + j0; a.ndraws = (int)nb;
                a.out = d.out; a.ld = d.ld; a.draw_stride = d.draw_stride; a.comp = d.comp; a.comp_stride = d.comp_stride;
                return launch_regress_draw_range(a, c->stream);
            });
        })) return rc;
    return skip_close(c, c->d_reg_skip, P, skipped);
}

int dpmm_regress_draw_points(dpmm_ctx *c, float *out, int64_t ld, int64_t draw_stride, int32_t *comp, uint64_t seed, int64_t i0, int64_t draw0, int64_t ndraws,
                             int64_t *skipped) {
    return regress_draw_points(c, out, ld, draw_stride, comp, seed, i0, draw0, ndraws, skipped, false, "dpmm_regress_draw_points");
}
int dpmm_regress_draw_points_device(dpmm_ctx *c, float *d_out, int64_t ld, int64_t draw_stride, int32_t *d_comp, uint64_t seed, int64_t i0, int64_t draw0,
                                    int64_t ndraws, int64_t *skipped) {
    return regress_draw_points(c, d_out, ld, draw_stride, d_comp, seed, i0, draw0, ndraws, skipped, true, "dpmm_regress_draw_points_device");
}

// ---- include/dpmm_hip_regress_cdf.h: conditional CDF and quantiles of the targets, range by range (regress_cdf.hip) --------------------------
int dpmm_set_regression_levels(dpmm_ctx *c, int L, const double *levels, const double *z) {
    static const char *fn = "dpmm_set_regression_levels";
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, who + "the regression is that of the NIW prior's Student-t predictive");
    if (L < 1 || L > DPMM_REGRESS_MAX_LEVELS) return fail(c, DPMM_EINVAL, who + "L must be in 1.." + std::to_string(DPMM_REGRESS_MAX_LEVELS));
    if (!levels || !z) return fail(c, DPMM_EINVAL, who + "null table");
    if (!c->predictive || c->reg_gen == 0 || c->reg_gen != c->pred_gen) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_regression for the predictive parameters in force");
    const size_t K = (size_t)c->K;
    for (int q = 0; q < L; ++q) {
        if (!(levels[q] > 0.0 && levels[q] < 1.0)) return fail(c, DPMM_EINVAL, who + "a level outside (0, 1)");
        if (q && !(levels[q] > levels[q - 1])) return fail(c, DPMM_EINVAL, who + "the levels must be strictly increasing");
    }
    for (size_t j = 0; j < K * (size_t)L; ++j)
        if (!std::isfinite(z[j])) return fail(c, DPMM_EINVAL, who + "a z that is not finite");
    HIPCHK(c, hipSetDevice(c->device));
    c->reg_lev_gen = 0;      // (a failure below leaves no levels in force)
    std::vector<double> img((size_t)L + K * (size_t)L + K);
    std::copy(levels, levels + L, img.begin());
    std::copy(z, z + K * (size_t)L, img.begin() + L);
    for (size_t k = 0; k < K; ++k) {      // log of the density of t_nu at 0: -log B(nu / 2, 1 / 2) - log(nu) / 2
        const double nu = (double)c->h_miss_cst[k * MISS_CST] + (double)c->D;
        img[(size_t)L + K * (size_t)L + k] = -typ_log_beta(0.5 * nu, 0.5) - 0.5 * std::log(nu);
    }
    if (int rc = grow(c, c->d_reg_lev, sizeof(double) * img.size(), fn, "regression levels")) return rc;
    HIPCHK(c, sync_stream(c, c->stream));
    HIPCHK(c, hipMemcpy(c->d_reg_lev, img.data(), sizeof(double) * img.size(), hipMemcpyHostToDevice));
    c->reg_L = L;
    c->reg_lev_gen = c->pred_gen;
    return DPMM_OK;
}

// Both calls: quant: the quantiles, out [n][L][ld]; else the CDF of y into out (cdf) and sf.  Host variants go through the staging block:
// per range y in, then the outputs dense (D_t apart).
static int regress_cdf_points(dpmm_ctx *c, const float *y, int64_t ldy, float *out, float *sf, int64_t ld, int64_t *labels, int64_t *skipped, bool quant,
                              bool device, const char *fn) {
    if (int rc = regress_front(c, fn, quant ? REGRESS_LEVELS : REGRESS_TABLES)) return rc;
    const std::string who = std::string(fn) + ": ";
    const int64_t Dt = c->reg_Dt, L = quant ? c->reg_L : 1;
    if (ld < Dt || (!quant && ldy < Dt)) return fail(c, DPMM_EINVAL, who + "ld < D_t");
    if ((ld >> 36) || (!quant && (ldy >> 40))) return fail(c, DPMM_EINVAL, who + "ld out of range");
    HIPCHK(c, hipSetDevice(c->device));
    if (skipped) skipped[0] = 0;
    if (c->n == 0) return DPMM_OK;
    if (!c->have_points || !c->have_params || !c->dX) return fail(c, DPMM_ESTATE, who + "needs points and parameters");
    if (!out) return fail(c, DPMM_EINVAL, who + (quant ? "out is null" : "cdf is null"));
    if (!quant && !y) return fail(c, DPMM_EINVAL, who + "y is null");
    // the rows: in the caller's device memory ld (ldy) floats apart, L rows a point; staged (host variants) dense, D_t apart.  y (null with
    // quant) comes first: its extent is the first one checked
    const size_t row = sizeof(float) * (size_t)Dt, pitch = sizeof(float) * (size_t)ld;
    OutStage<4> st{{{const_cast<float *>(y), "d_y", 4, row, sizeof(float) * (size_t)ldy, 1, true}, {out, quant ? "d_out" : "d_cdf", 4, row, pitch, (size_t)L},
                    {sf, "d_sf", 4, row, pitch}, {labels, "d_labels", 8, sizeof(int64_t)}}, device};
    if (int rc = st.check(c, fn, (uint64_t)c->n)) return rc;
    TableWalk w;
    if (int rc = walk_open(c, fn, WALK_MISS_NEVER, &w)) return rc;
    if (int rc = skip_open(c, c->d_reg_skip, w.P, fn, "counts of the regression pass")) return rc;
    if (int rc = st.open(c, w.P)) return rc;
    const double *lev = c->d_reg_lev;
    if (int rc = walk_ranges(c, w, c->n, fn, [&](int64_t p0, int64_t np, int64_t) {
            const RegressTile t = regress_tile(c, w.P, p0, np, st.at<int64_t>(3, p0), c->d_reg_skip);
            hipError_t e = device ? hipSuccess : st.load(c, p0, (size_t)np);
            if (e != hipSuccess) return e;
            if (quant) {
                RegressQuantileArgs a = regress_flat_args<RegressQuantileArgs>(c, t);
                a.levels = lev; a.z = lev + L; a.lc = lev + L + (int64_t)c->K * L; a.L = (int)L;
                a.out = st.at<float>(1, p0); a.ld = device ? ld : Dt;
                e = launch_regress_quantile_range(a, c->stream);
            } else {
                RegressCdfArgs a = regress_flat_args<RegressCdfArgs>(c, t);
                a.y = st.at<float>(0, p0); a.ldy = device ? ldy : Dt;
                a.cdf = st.at<float>(1, p0); a.sf = st.at<float>(2, p0); a.ld = device ? ld : Dt;
                e = launch_regress_cdf_range(a, c->stream);
            }
            if (e == hipSuccess && !device) e = st.flush(c, p0, (size_t)np);
            return e;
        })) return rc;
    return skip_close(c, c->d_reg_skip, w.P, skipped);
}

int dpmm_regress_cdf_points(dpmm_ctx *c, const float *y, int64_t ldy, float *cdf, float *sf, int64_t ld, int64_t *labels, int64_t *skipped) {
    return regress_cdf_points(c, y, ldy, cdf, sf, ld, labels, skipped, false, false, "dpmm_regress_cdf_points");
}
int dpmm_regress_cdf_points_device(dpmm_ctx *c, const float *d_y, int64_t ldy, float *d_cdf, float *d_sf, int64_t ld, int64_t *d_labels, int64_t *skipped) {
    return regress_cdf_points(c, d_y, ldy, d_cdf, d_sf, ld, d_labels, skipped, false, true, "dpmm_regress_cdf_points_device");
}
int dpmm_regress_quantile_points(dpmm_ctx *c, float *out, int64_t ld, int64_t *labels, int64_t *skipped) {
    return regress_cdf_points(c, nullptr, 0, out, nullptr, ld, labels, skipped, true, false, "dpmm_regress_quantile_points");
}
int dpmm_regress_quantile_points_device(dpmm_ctx *c, float *d_out, int64_t ld, int64_t *d_labels, int64_t *skipped) {
    return regress_cdf_points(c, nullptr, 0, d_out, nullptr, ld, d_labels, skipped, true, true, "dpmm_regress_quantile_points_device");
}

// ---- include/dpmm_hip_rank.h: exemplars, the m most and least typical points of every cluster (rank.hip) -----------------------------------
static size_t rank_keys_words(int K) { return (size_t)2 * (size_t)K * RANK_SLOTS; }
static size_t rank_count_words(int K) { return (size_t)RANK_REPL * (size_t)(K + 1); }
// the outputs of dpmm_rank_read in the order of dpmm_rank_out, one element per column: the whole array (launch_rank_read writes all six)
static OutStage<6> rank_out_stage(const dpmm_rank_out &o, int K, int m, bool device) {
    const size_t km = (size_t)K * (size_t)m;
    return {{{o.typ_idx, "typ_idx", 8, sizeof(int64_t) * km}, {o.typ_score, "typ_score", 4, sizeof(float) * km}, {o.fringe_idx, "fringe_idx", 8, sizeof(int64_t) * km},
             {o.fringe_score, "fringe_score", 4, sizeof(float) * km}, {o.count, "count", 8, sizeof(int64_t) * (size_t)K}, {o.skipped, "skipped", 8, sizeof(int64_t)}},
            device, true};
}

int dpmm_rank_begin(dpmm_ctx *c, int m, int which) {
    static const char *fn = "dpmm_rank_begin";
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (m < 1 || m > DPMM_RANK_MAX_M) return fail(c, DPMM_EINVAL, who + "m must be in 1.." + std::to_string(DPMM_RANK_MAX_M));
    if (which < 1 || which > (DPMM_RANK_TYPICAL | DPMM_RANK_FRINGE)) return fail(c, DPMM_EINVAL, who + "which must be DPMM_RANK_TYPICAL, DPMM_RANK_FRINGE or both");
    if (!c->predictive) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_predictive_* first");
    HIPCHK(c, hipSetDevice(c->device));
    c->rank_active = false;
    const int K = c->K;
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(RANK_CHUNK, c->n));
    const size_t state = sizeof(unsigned long long) * (rank_keys_words(K) + rank_count_words(K) + 2);      // (2 words: the four candidate counters)
    const size_t cand = (size_t)2 * (size_t)cap * (sizeof(unsigned long long) + sizeof(uint16_t));
    const size_t out = rank_out_stage(dpmm_rank_out{}, K, m, false).layout(1);
    if (int rc = grow(c, c->d_rank_state, state, "dpmm_score_points", "running lists of dpmm_rank_begin")) return rc;
    if (int rc = grow(c, c->d_rank_cand, cand, "dpmm_score_points", "candidate buffers of dpmm_rank_begin")) return rc;
    if (int rc = grow(c, c->d_rank_out, out, "dpmm_score_points", "staging of dpmm_rank_read")) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_rank_state, 0, state, c->stream));
    c->rank_m = m; c->rank_which = which; c->rank_K = K; c->rank_cap = cap; c->rank_parity = 0;
    c->rank_active = true;
    return DPMM_OK;
}

int dpmm_rank_accumulate(dpmm_ctx *c, int64_t index_base, int64_t n_valid) {
    static const char *fn = "dpmm_rank_accumulate";
    if (!c) return tensor_no_ctx(fn);
    c->miss_counted = false;      // (as score_points)
    const std::string who = std::string(fn) + ": ";
    if (!c->rank_active) return fail(c, DPMM_ESTATE, who + "needs dpmm_rank_begin first");
    if (!c->predictive || c->K != c->rank_K) return fail(c, DPMM_ESTATE, who + "the predictive parameters changed since dpmm_rank_begin");
    if (n_valid < 0 || n_valid > c->n) return fail(c, DPMM_EINVAL, who + "n_valid must be in 0..n_local");
    if (index_base < 0 || index_base > ((int64_t)1 << 32) - n_valid) return fail(c, DPMM_EINVAL, who + "global indices must lie in 0..2^32 - 1");
    HIPCHK(c, hipSetDevice(c->device));
    if (n_valid == 0) return DPMM_OK;
    if (!c->have_points || !c->have_params) return fail(c, DPMM_ESTATE, who + "needs points and parameters");
    if (c->rank_cap < std::min<int64_t>(RANK_CHUNK, c->n)) return fail(c, DPMM_ESTATE, who + "the context's points changed since dpmm_rank_begin");
    TableWalk w;
    if (int rc = walk_open(c, fn, WALK_MISS_OPTION, &w)) return rc;
    const int K = c->K;
    unsigned long long *keys = c->d_rank_state, *count = keys + rank_keys_words(K);
    unsigned *cand_n = reinterpret_cast<unsigned *>(count + rank_count_words(K));
    unsigned long long *cand_key = reinterpret_cast<unsigned long long *>(c->d_rank_cand.get());
    uint16_t *cand_k = reinterpret_cast<uint16_t *>(cand_key + 2 * c->rank_cap);
    return walk_ranges(c, w, n_valid, fn, [&](int64_t p0, int64_t, int64_t nv) {
        hipError_t e = hipSuccess;
        for (int64_t q0 = 0; q0 < nv && e == hipSuccess; q0 += c->rank_cap) {
            RankArgs a{};
            a.table = c->d_score_table + q0; a.stride = w.P; a.rstep = w.rstep; a.n = std::min<int64_t>(c->rank_cap, nv - q0); a.K = K;
            a.index0 = index_base + p0 + q0; a.m = c->rank_m; a.which = c->rank_which;
            a.keys = keys; a.count = count; a.cand_key = cand_key; a.cand_k = cand_k; a.cand_n = cand_n; a.cap = c->rank_cap; a.parity = c->rank_parity;
            e = launch_rank_chunk(a, c->stream);
            if (e == hipSuccess) c->rank_parity ^= 1;
        }
        return e;
    });
}

static int rank_read(dpmm_ctx *c, const dpmm_rank_out *o, bool device, const char *fn) {
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (!o) return fail(c, DPMM_EINVAL, who + "out is null");
    if (!c->rank_active) return fail(c, DPMM_ESTATE, who + "needs dpmm_rank_begin first");
    HIPCHK(c, hipSetDevice(c->device));
    const int K = c->rank_K, m = c->rank_m;
    OutStage<6> out = rank_out_stage(*o, K, m, device);
    if (int rc = out.check(c, fn, 1)) return rc;
    out.layout(1);
    out.buf = c->d_rank_out;      // (dpmm_rank_begin sized it)
    const RankOut r{out.at<int64_t>(0, 0), out.at<float>(1, 0), out.at<int64_t>(2, 0), out.at<float>(3, 0), out.at<int64_t>(4, 0), out.at<int64_t>(5, 0)};
    const unsigned long long *keys = c->d_rank_state, *count = keys + rank_keys_words(K);
    hipError_t e = launch_rank_read(keys, count, K, m, c->rank_which, r, c->stream);
    if (e == hipSuccess) e = device ? sync_stream(c, c->stream) : out.flush(c, 0, 1);
    return table_result(c, fn, e);
}

int dpmm_rank_read(dpmm_ctx *c, const dpmm_rank_out *out) { return rank_read(c, out, false, "dpmm_rank_read"); }
int dpmm_rank_read_device(dpmm_ctx *c, const dpmm_rank_out *out) { return rank_read(c, out, true, "dpmm_rank_read_device"); }

// ---- what the accumulations over the table share (overlap, batchstats, holdout, countstats, countholdout): the session record, the fronts of
// their _accumulate and _read calls, the second floor, the count data's point store and the replicated counters ---------------------------
// an _accumulate call: its *_begin has run, and under the parameters in force now
static int session_check(dpmm_ctx *c, const AccSession &s, const char *begin_name, const char *fn) {
    if (!s.active) return fail(c, DPMM_ESTATE, std::string(fn) + ": needs " + begin_name + " first");
    if (!c->predictive || c->K != s.K || c->pred_gen != s.gen) return fail(c, DPMM_ESTATE, std::string(fn) + ": the predictive parameters changed since " + begin_name);
    return DPMM_OK;
}
// The live point store as the count kernels name it, and whether its buffers are there
static int count_store(const dpmm_ctx *c) { return c->x_sparse ? COUNTSTATS_SPARSE : c->x_u8 ? COUNTSTATS_U8 : COUNTSTATS_F32; }
static bool count_store_ready(const dpmm_ctx *c, int store) {
    const bool have = store == COUNTSTATS_SPARSE ? (bool)c->d_cp : store == COUNTSTATS_U8 ? (bool)c->dX8 : (bool)c->dX;
    return c->have_points && c->have_params && have && !(store == COUNTSTATS_SPARSE && c->nnz > 0 && (!c->d_ri || !c->d_val));
}
// ... and the points from p0 on, in the members every argument struct of the count kernels has (CountTotalsArgs reads no rows: no `ri`)
extern "C++" {
template <class Args> static auto count_rows(Args &a, const uint16_t *ri, int) -> decltype((void)(a.ri = ri)) { a.ri = ri; }
template <class Args> static void count_rows(Args &, const uint16_t *, long) {}
template <class Args>
static void count_points(const dpmm_ctx *c, int store, int64_t p0, Args &a) {
    a.store = store;
    if (store == COUNTSTATS_SPARSE) { a.cp = c->d_cp + p0; count_rows(a, c->d_ri, 0); a.val = c->d_val; }
    else if (store == COUNTSTATS_U8) { a.X8 = c->dX8 + p0 * c->ld8; a.ld8 = c->ld8; }
    else { a.X = c->dX + p0 * c->ldx; a.ldx = c->ldx; }
}
}  // extern "C++"
// The front of an _accumulate call, in the order the headers state: session, n_valid, lo (the calls that take one), device, nothing to do
// (*empty), points and parameters.  What a call checks beyond these follows at its own place.
enum AccPoints { ACC_POINTS, ACC_DENSE, ACC_COUNTS };      // the points it reads: through the table only | the Float32 matrix | the live count store
static int acc_front(dpmm_ctx *c, AccSession dpmm_ctx::*session, const char *begin_name, const char *fn, int64_t n_valid, const int64_t *lo, AccPoints need,
                     bool *empty) {
    if (!c) return tensor_no_ctx(fn);
    c->miss_counted = false;      // (as score_points)
    const std::string who = std::string(fn) + ": ";
    if (int rc = session_check(c, c->*session, begin_name, fn)) return rc;
    if (n_valid < 0 || n_valid > c->n) return fail(c, DPMM_EINVAL, who + "n_valid must be in 0..n_local");
    if (lo && (*lo < 0 || *lo > ((int64_t)1 << 62) - n_valid)) return fail(c, DPMM_EINVAL, who + "global indices must lie in 0..2^62");
    HIPCHK(c, hipSetDevice(c->device));
    *empty = n_valid == 0;
    if (*empty) return DPMM_OK;
    const bool ready = need == ACC_COUNTS ? count_store_ready(c, count_store(c)) : c->have_points && c->have_params && (need == ACC_POINTS || c->dX);
    if (!ready) return fail(c, DPMM_ESTATE, who + "needs points and parameters");
    return DPMM_OK;
}
// The front of a _read call
static int read_front(dpmm_ctx *c, AccSession dpmm_ctx::*session, const char *begin_name, const char *fn, const void *out) {
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (!out) return fail(c, DPMM_EINVAL, who + "out is null");
    if (!(c->*session).active) return fail(c, DPMM_ESTATE, who + "needs " + begin_name + " first");
    HIPCHK(c, hipSetDevice(c->device));
    return DPMM_OK;
}
// The second floor of the statistics just begun (`family`: dpmm_batchstats / dpmm_countstats); `bad`: what is wrong with the value, or null
static int set_second_floor(dpmm_ctx *c, AccSession dpmm_ctx::*session, const std::string &family, const char *fn, int use, float v, const char *bad) {
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    AccSession &s = c->*session;
    if (!s.active) return fail(c, DPMM_ESTATE, who + "needs " + family + "_begin first");
    if (s.accumulated) return fail(c, DPMM_ESTATE, who + "belongs between " + family + "_begin and the first " + family + "_accumulate");
    if (use && bad) return fail(c, DPMM_EINVAL, who + bad);
    s.use2 = use ? 1 : 0;
    s.min2 = use ? v : 0.f;
    return DPMM_OK;
}
// counter k of RANK_REPL replicas, `stride` words apart (a workgroup adds to one replica)
static int64_t fold_replicated(const std::vector<unsigned long long> &cnt, size_t stride, size_t k) {
    unsigned long long v = 0;
    for (int r = 0; r < RANK_REPL; ++r) v += cnt[(size_t)r * stride + k];
    return (int64_t)v;
}
static const char *const RANGE_TOO_LONG = "a range of the table must hold fewer than 2^31 points: lower DPMM_OPT_SCORE_TABLE_MB";

// ---- include/dpmm_hip_overlap.h: the posterior overlap of the clusters, sum_i p_ik p_ij (overlap.hip) --------------------------------------
static size_t overlap_acc_doubles(int K) { return (size_t)K * (size_t)K + (size_t)K; }
static int overlap_max_chunks(int K) { const int nb = (K + 63) / 64, np = nb * (nb + 1) / 2; return std::max(1, OVERLAP_PARTIAL_BLOCKS / np); }

int dpmm_overlap_begin(dpmm_ctx *c) {
    static const char *fn = "dpmm_overlap_begin";
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (!c->predictive) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_predictive_* first");
    HIPCHK(c, hipSetDevice(c->device));
    c->ov.active = false;
    const int K = c->K, nb = (K + 63) / 64, npairs = nb * (nb + 1) / 2;
    const size_t state = sizeof(double) * overlap_acc_doubles(K) + sizeof(unsigned long long) * rank_count_words(K);
    const size_t part = sizeof(double) * (size_t)overlap_max_chunks(K) * ((size_t)npairs * 4096 + (size_t)nb * 64);
    if (int rc = grow(c, c->d_ov_acc, state, "dpmm_score_points", "accumulators of dpmm_overlap_begin")) return rc;
    if (int rc = grow(c, c->d_ov_part, part, "dpmm_score_points", "chunk partials of dpmm_overlap_begin")) return rc;
    if (c->n > 0) {      // (M, S) of one range: sized as dpmm_overlap_accumulate will find it unless the table budget changes in between
        int rstep = 0;
        int64_t P = 0;
        if (int rc = score_table_slab(c, &rstep, &P)) return rc;
        if (int rc = grow(c, c->d_ov_ms, sizeof(float2) * (size_t)P, "dpmm_score_points", "maxima and sums of dpmm_overlap_begin")) return rc;
    }
    HIPCHK(c, hipMemsetAsync(c->d_ov_acc, 0, state, c->stream));
    c->ov = AccSession{true, K, 0, 0, 0.f, c->pred_gen};
    return DPMM_OK;
}

int dpmm_overlap_accumulate(dpmm_ctx *c, int64_t n_valid) {
    static const char *fn = "dpmm_overlap_accumulate";
    bool empty = false;
    if (int rc = acc_front(c, &dpmm_ctx::ov, "dpmm_overlap_begin", fn, n_valid, nullptr, ACC_POINTS, &empty)) return rc;
    if (empty) return DPMM_OK;
    const std::string who = std::string(fn) + ": ";
    TableWalk w;
    if (int rc = walk_open(c, fn, WALK_MISS_OPTION, &w, [&](int64_t P) {
            return grow(c, c->d_ov_ms, sizeof(float2) * (size_t)P, "dpmm_score_points", "maxima and sums of dpmm_overlap_accumulate");
        })) return rc;
    const int K = c->K, nb = (K + 63) / 64, npairs = nb * (nb + 1) / 2;
    const int most = overlap_max_chunks(K);
    return walk_ranges(c, w, n_valid, fn, [&](int64_t, int64_t, int64_t nv) -> int {
        OverlapArgs a{};
        a.table = c->d_score_table; a.stride = w.P; a.rstep = w.rstep; a.n = nv; a.K = K; a.nb = nb;
        overlap_chunks(a.n, K, &a.nchunk, &a.chunk);
        if (a.nchunk > most) return fail(c, DPMM_EHIP, who + "internal: more chunks than the partial buffer holds");
        a.ms = c->d_ov_ms;
        a.acc = c->d_ov_acc;
        a.count = reinterpret_cast<unsigned long long *>(c->d_ov_acc + overlap_acc_doubles(K));
        a.part = c->d_ov_part;
        a.mpart = c->d_ov_part + (size_t)most * (size_t)npairs * 4096;
        return table_result(c, fn, launch_overlap_range(a, c->stream));
    });
}

int dpmm_overlap_read(dpmm_ctx *c, const dpmm_overlap_out *o) {
    static const char *fn = "dpmm_overlap_read";
    if (int rc = read_front(c, &dpmm_ctx::ov, "dpmm_overlap_begin", fn, o)) return rc;
    const int K = c->ov.K;
    const size_t kk = (size_t)K * (size_t)K;
    std::vector<unsigned long long> cnt(rank_count_words(K));
    hipError_t e = sync_stream(c, c->stream);
    if (e == hipSuccess && o->overlap) e = hipMemcpy(o->overlap, c->d_ov_acc, sizeof(double) * kk, hipMemcpyDeviceToHost);
    if (e == hipSuccess && o->mass) e = hipMemcpy(o->mass, c->d_ov_acc + kk, sizeof(double) * (size_t)K, hipMemcpyDeviceToHost);
    if (e == hipSuccess && (o->count || o->skipped)) e = hipMemcpy(cnt.data(), c->d_ov_acc + overlap_acc_doubles(K), sizeof(unsigned long long) * cnt.size(), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { c->err = std::string(fn) + ": " + hipGetErrorString(e); return DPMM_EHIP; }
    if (o->count) for (int k = 0; k < K; ++k) o->count[k] = fold_replicated(cnt, (size_t)K + 1, (size_t)k);
    if (o->skipped) o->skipped[0] = fold_replicated(cnt, (size_t)K + 1, (size_t)K);
    return DPMM_OK;
}

// ---- include/dpmm_hip_batchstats.h: per-cluster sufficient statistics of a batch, sum_i w_ik (1, x_i, x_i x_i') (batchstats.hip) -----------
static size_t batchstats_acc_doubles(int K, int D) { return (size_t)K * ((size_t)D * (size_t)D + (size_t)D + 1); }
static size_t batchstats_count_words(int K) { return (size_t)RANK_REPL * (size_t)(K + BATCHSTATS_COUNTERS); }
// The tail of dpmm_batchstats_read and dpmm_countstats_read: e, the result of the copies so far; d_cnt, the session's counters
// count[K] | skipped | held out | incomplete behind its accumulators.  Read only if one of them is asked for.
static int stats_counters_read(dpmm_ctx *c, const char *fn, hipError_t e, const double *d_cnt, int K, int64_t *count, int64_t *skipped, int64_t *held_out,
                               int64_t *incomplete) {
    std::vector<unsigned long long> cnt(batchstats_count_words(K));
    if (e == hipSuccess && (count || skipped || incomplete || held_out)) e = hipMemcpy(cnt.data(), d_cnt, sizeof(unsigned long long) * cnt.size(), hipMemcpyDeviceToHost);
    if (int rc = table_result(c, fn, e)) return rc;
    const size_t stride = (size_t)K + BATCHSTATS_COUNTERS;
    if (count) for (int k = 0; k < K; ++k) count[k] = fold_replicated(cnt, stride, (size_t)k);
    if (skipped) skipped[0] = fold_replicated(cnt, stride, (size_t)K);
    if (held_out) held_out[0] = fold_replicated(cnt, stride, (size_t)K + 1);
    if (incomplete) incomplete[0] = fold_replicated(cnt, stride, (size_t)K + 2);
    return DPMM_OK;
}
// doubles of the chunk partials of a range of at most `len` points: blocks | rows of sums | weights (the offsets of the three parts)
static size_t batchstats_part_doubles(int64_t len, int K, int D, size_t *off_s, size_t *off_n) {
    const int nb = (D + 63) / 64, npairs = nb * (nb + 1) / 2;
    int kg = 0, nchunk = 0;
    int64_t chunk = 0;
    batchstats_chunks(len, K, D, &kg, &nchunk, &chunk);
    const size_t most = (size_t)std::max(1, BATCHSTATS_PARTIAL_BLOCKS / (kg * npairs));
    const size_t ck = std::min<size_t>(most, (size_t)std::max<int64_t>(1, (len + 2047) / 2048)) * (size_t)kg;      // (chunks, cluster) at most
    *off_s = ck * (size_t)npairs * 4096;
    *off_n = ck * (size_t)npairs * 4096 + ck * (size_t)nb * 64;
    return ck * ((size_t)npairs * 4096 + (size_t)nb * 64 + 1);
}
// one range of P points: its two floats per point and its chunk partials, grown; the offsets of the partials' parts
static int batchstats_range_buffers(dpmm_ctx *c, int64_t P, size_t *off_s, size_t *off_n) {
    const size_t part = sizeof(double) * batchstats_part_doubles(std::min<int64_t>(P, c->n), c->K, c->D, off_s, off_n);
    if (int rc = grow(c, c->d_bs_ms, sizeof(float2) * (size_t)P, "dpmm_score_points", "maxima and sums of the batch statistics")) return rc;
    return grow(c, c->d_bs_part, part, "dpmm_score_points", "chunk partials of the batch statistics");
}

int dpmm_batchstats_begin(dpmm_ctx *c, int mode, int use_floor, float min_logdens) {
    static const char *fn = "dpmm_batchstats_begin";
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, who + "the statistics are those of the NIW prior; a Multinomial ctx has dpmm_countstats_begin / _accumulate / _read (include/dpmm_hip_countstats.h)");
    if (mode != DPMM_BATCHSTATS_HARD && mode != DPMM_BATCHSTATS_SOFT) return fail(c, DPMM_EINVAL, who + "mode must be DPMM_BATCHSTATS_HARD or DPMM_BATCHSTATS_SOFT");
    if (!c->predictive) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_predictive_niw first");
    HIPCHK(c, hipSetDevice(c->device));
    c->bs.active = false;
    const int K = c->K, D = c->D;
    const size_t state = sizeof(double) * batchstats_acc_doubles(K, D) + sizeof(unsigned long long) * batchstats_count_words(K);
    if (int rc = grow(c, c->d_bs_acc, state, "dpmm_score_points", "accumulators of dpmm_batchstats_begin")) return rc;
    if (c->n > 0) {      // one range's floats and partials: sized as dpmm_batchstats_accumulate will find them unless the table budget changes in between
        int rstep = 0;
        int64_t P = 0;
        size_t off_s = 0, off_n = 0;
        if (int rc = score_table_slab(c, &rstep, &P)) return rc;
        if (int rc = batchstats_range_buffers(c, P, &off_s, &off_n)) return rc;
    }
    HIPCHK(c, hipMemsetAsync(c->d_bs_acc, 0, state, c->stream));
    c->bs = AccSession{true, K, mode, use_floor ? 1 : 0, min_logdens, c->pred_gen};
    return DPMM_OK;
}

// include/dpmm_hip_typicality.h: the calibrated floor of the accumulation just begun
int dpmm_batchstats_set_min_tail(dpmm_ctx *c, int use, float min_tail) {
    return set_second_floor(c, &dpmm_ctx::bs, "dpmm_batchstats", "dpmm_batchstats_set_min_tail", use, min_tail,
                            min_tail > 0.f && min_tail <= 1.f ? nullptr : "min_tail must lie in (0, 1]");
}

int dpmm_batchstats_accumulate(dpmm_ctx *c, int64_t n_valid) {
    static const char *fn = "dpmm_batchstats_accumulate";
    bool empty = false;
    if (int rc = acc_front(c, &dpmm_ctx::bs, "dpmm_batchstats_begin", fn, n_valid, nullptr, ACC_DENSE, &empty)) return rc;
    if (empty) return DPMM_OK;
    const std::string who = std::string(fn) + ": ";
    const int K = c->K, D = c->D;
    size_t off_s = 0, off_n = 0;
    TableWalk w;
    if (int rc = walk_open(c, fn, WALK_MISS_OPTION, &w, [&](int64_t P) -> int {
            if (P >> 31) return fail(c, DPMM_EINVAL, who + RANGE_TOO_LONG);
            return batchstats_range_buffers(c, P, &off_s, &off_n);
        })) return rc;
    if (c->bs.use2) {
        if (int rc = grow(c, c->d_bs_tail, sizeof(float) * (size_t)w.P, "dpmm_score_points", "tails of dpmm_batchstats_accumulate")) return rc;
        if (int rc = typ_begin(c, w.P, fn)) return rc;
    }
    c->bs.accumulated = true;
    return walk_ranges(c, w, n_valid, fn, [&](int64_t p0, int64_t, int64_t nv) -> int {
        if (c->bs.use2) if (int rc = typ_range(c, w.P, p0, nv, nullptr, nullptr, c->d_bs_tail, fn)) return rc;
        BatchStatsArgs a{};
        a.table = c->d_score_table; a.stride = w.P; a.rstep = w.rstep; a.n = nv; a.K = K; a.D = D; a.nb = (D + 63) / 64;
        a.X = c->dX + p0 * c->ldx; a.ldx = c->ldx;
        a.soft = c->bs.mode == DPMM_BATCHSTATS_SOFT; a.use_floor = c->bs.floor; a.min_logdens = c->bs.min_logdens;
        a.use_tail = c->bs.use2; a.min_tail = c->bs.min2; a.tail = c->bs.use2 ? c->d_bs_tail.get() : nullptr;
        batchstats_chunks(a.n, K, D, &a.kgroup, &a.nchunk, &a.chunk);
        if ((size_t)a.nchunk * (size_t)std::min(a.kgroup, K) * (size_t)(a.nb * (a.nb + 1) / 2) * 4096 > off_s)
            return fail(c, DPMM_EHIP, who + "internal: more chunks than the partial buffer holds");
        a.ms = c->d_bs_ms;
        a.acc = c->d_bs_acc;
        a.count = reinterpret_cast<unsigned long long *>(c->d_bs_acc + batchstats_acc_doubles(K, D));
        a.part = c->d_bs_part;
        a.spart = c->d_bs_part + off_s;
        a.npart = c->d_bs_part + off_n;
        return table_result(c, fn, launch_batchstats_range(a, c->stream));
    });
}

int dpmm_batchstats_read(dpmm_ctx *c, const dpmm_batchstats_out *o) {
    static const char *fn = "dpmm_batchstats_read";
    if (int rc = read_front(c, &dpmm_ctx::bs, "dpmm_batchstats_begin", fn, o)) return rc;
    const int K = c->bs.K;
    const size_t D = (size_t)c->D, Kz = (size_t)K;
    hipError_t e = sync_stream(c, c->stream);
    if (e == hipSuccess && o->N) e = hipMemcpy(o->N, c->d_bs_acc, sizeof(double) * Kz, hipMemcpyDeviceToHost);
    if (e == hipSuccess && o->sums) e = hipMemcpy(o->sums, c->d_bs_acc + Kz, sizeof(double) * Kz * D, hipMemcpyDeviceToHost);
    if (e == hipSuccess && o->S) e = hipMemcpy(o->S, c->d_bs_acc + Kz + Kz * D, sizeof(double) * Kz * D * D, hipMemcpyDeviceToHost);
    return stats_counters_read(c, fn, e, c->d_bs_acc + batchstats_acc_doubles(K, (int)D), K, o->count, o->skipped, o->held_out, o->incomplete);
}

// ---- include/dpmm_hip_holdout.h: the held-out points of the batch, compacted into the caller's device memory (holdout.hip) -----------------
static int holdout_check_dst(dpmm_ctx *c, const char *fn, float *points, int64_t *index, int64_t cap) {
    if (cap <= 0) return DPMM_OK;
    if (int rc = check_device_extent(c, fn, "dst_points", points, (uint64_t)cap * (uint64_t)c->D * sizeof(float), sizeof(float))) return rc;
    return check_device_extent(c, fn, "dst_index", index, (uint64_t)cap * sizeof(int64_t), sizeof(int64_t));
}
// one range of P points: the ballots, class counts and first slots of its workgroups, grown; entries (count data): their entry counts and
// first entry offsets too
static int holdout_range_buffers(dpmm_ctx *c, int64_t P, bool entries) {
    const size_t groups = (size_t)holdout_groups(std::min<int64_t>(P, c->n));
    if (int rc = grow(c, c->d_ho_ballot, sizeof(unsigned long long) * groups * (HOLDOUT_THREADS / 64), "dpmm_score_points", "ballots of the held-out points")) return rc;
    if (int rc = grow(c, c->d_ho_count, sizeof(unsigned) * groups * HOLDOUT_STATE, "dpmm_score_points", "workgroup counts of the held-out points")) return rc;
    if (entries) {
        if (int rc = grow(c, c->d_ch_ent, sizeof(unsigned long long) * groups, "dpmm_score_points", "workgroup entry counts of the held-out points")) return rc;
        if (int rc = grow(c, c->d_ch_eoff, sizeof(int64_t) * groups, "dpmm_score_points", "workgroup entry offsets of the held-out points")) return rc;
    }
    return grow(c, c->d_ho_off, sizeof(int64_t) * groups, "dpmm_score_points", "workgroup slots of the held-out points");
}

int dpmm_holdout_begin(dpmm_ctx *c, int use_floor, float min_logdens, int use_tail, float min_tail, float *dst_points, int64_t *dst_index, int64_t cap) {
    static const char *fn = "dpmm_holdout_begin";
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, who + "held-out points are collected under the NIW prior and from dense points; a Multinomial ctx is out of scope");
    if (!use_floor && !use_tail) return fail(c, DPMM_EINVAL, who + "needs a floor: use_floor or use_tail");
    if (use_tail && !(min_tail > 0.f && min_tail <= 1.f)) return fail(c, DPMM_EINVAL, who + "min_tail must lie in (0, 1]");
    if (cap < 0 || (cap >> 40)) return fail(c, DPMM_EINVAL, who + "cap must be in 0..2^40 - 1");
    if (!c->predictive) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_predictive_niw first");
    HIPCHK(c, hipSetDevice(c->device));
    c->ho.active = false;
    if (int rc = holdout_check_dst(c, fn, dst_points, dst_index, cap)) return rc;
    if (int rc = grow(c, c->d_ho_state, sizeof(unsigned long long) * HOLDOUT_STATE, "dpmm_score_points", "counters of dpmm_holdout_begin")) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_ho_state, 0, sizeof(unsigned long long) * HOLDOUT_STATE, c->stream));
    c->ho = AccSession{true, c->K, 0, use_floor ? 1 : 0, min_logdens, c->pred_gen, use_tail ? 1 : 0, use_tail ? min_tail : 0.f};
    c->ho_points = dst_points; c->ho_index = dst_index; c->ho_cap = cap;
    return DPMM_OK;
}

int dpmm_holdout_accumulate(dpmm_ctx *c, int64_t lo, int64_t n_valid) {
    static const char *fn = "dpmm_holdout_accumulate";
    bool empty = false;
    if (int rc = acc_front(c, &dpmm_ctx::ho, "dpmm_holdout_begin", fn, n_valid, &lo, ACC_DENSE, &empty)) return rc;
    if (empty) return DPMM_OK;
    const std::string who = std::string(fn) + ": ";
    if (int rc = holdout_check_dst(c, fn, c->ho_points, c->ho_index, c->ho_cap)) return rc;      // (the caller may have freed it since the begin)
    TableWalk w;
    if (int rc = walk_open(c, fn, WALK_MISS_OPTION, &w, [&](int64_t P) -> int {
            if (P >> 31) return fail(c, DPMM_EINVAL, who + RANGE_TOO_LONG);
            return holdout_range_buffers(c, P, false);
        })) return rc;
    if (c->ho.use2) {
        if (int rc = grow(c, c->d_bs_tail, sizeof(float) * (size_t)w.P, "dpmm_score_points", "tails of dpmm_holdout_accumulate")) return rc;
        if (int rc = typ_begin(c, w.P, fn)) return rc;
    }
    return walk_ranges(c, w, n_valid, fn, [&](int64_t p0, int64_t, int64_t nv) -> int {
        if (c->ho.use2) if (int rc = typ_range(c, w.P, p0, nv, nullptr, nullptr, c->d_bs_tail, fn)) return rc;
        HoldoutArgs a{};
        a.table = c->d_score_table; a.stride = w.P; a.rstep = w.rstep; a.n = nv; a.K = c->K; a.D = c->D;
        a.X = c->dX + p0 * c->ldx; a.ldx = c->ldx;
        a.use_floor = c->ho.floor; a.min_logdens = c->ho.min_logdens;
        a.use_tail = c->ho.use2; a.min_tail = c->ho.min2; a.tail = c->ho.use2 ? c->d_bs_tail.get() : nullptr;
        a.index0 = lo + p0;
        a.ballot = c->d_ho_ballot; a.wgcount = c->d_ho_count; a.wgoff = c->d_ho_off; a.state = c->d_ho_state;
        a.dst_points = c->ho_points; a.dst_index = c->ho_index; a.cap = c->ho_cap;
        return table_result(c, fn, launch_holdout_range(a, c->stream));
    });
}

int dpmm_holdout_read(dpmm_ctx *c, const dpmm_holdout_out *o) {
    static const char *fn = "dpmm_holdout_read";
    if (int rc = read_front(c, &dpmm_ctx::ho, "dpmm_holdout_begin", fn, o)) return rc;
    unsigned long long h[HOLDOUT_STATE] = {0, 0, 0, 0};
    hipError_t e = sync_stream(c, c->stream);
    if (e == hipSuccess) e = hipMemcpy(h, c->d_ho_state, sizeof(h), hipMemcpyDeviceToHost);
    if (int rc = table_result(c, fn, e)) return rc;
    if (o->total) o->total[0] = (int64_t)h[0];
    if (o->stored) o->stored[0] = std::min<int64_t>((int64_t)h[0], c->ho_cap);
    if (o->skipped) o->skipped[0] = (int64_t)h[1];
    if (o->incomplete) o->incomplete[0] = (int64_t)h[2];
    if (o->scored) o->scored[0] = (int64_t)h[3];
    return DPMM_OK;
}

// ---- include/dpmm_hip_countstats.h: per-cluster count statistics of a batch under the Multinomial model, sum_i w_ik (1, x_i) (countstats.hip)
static size_t countstats_acc_doubles(int K, int D) { return (size_t)K * ((size_t)D + 1); }
// one range of P points: its two floats per point and its chunk partials -- rows of dp doubles | one weight per row -- grown; the partials' bytes
static int countstats_range_buffers(dpmm_ctx *c, int64_t P, size_t *part) {
    int kg = 0, nchunk = 0;
    int64_t chunk = 0, dp = 0;
    countstats_chunks(std::min<int64_t>(P, c->n), c->K, c->D, c->x_sparse ? 1 : 0, &kg, &nchunk, &chunk, &dp);
    *part = sizeof(double) * (size_t)nchunk * (size_t)kg * ((size_t)dp + 1);
    if (int rc = grow(c, c->d_cs_ms, sizeof(float2) * (size_t)P, "dpmm_score_points", "maxima and sums of the count statistics")) return rc;
    return grow(c, c->d_cs_part, *part, "dpmm_score_points", "chunk partials of the count statistics");
}

int dpmm_countstats_begin(dpmm_ctx *c, int mode, int use_floor, float min_logdens) {
    static const char *fn = "dpmm_countstats_begin";
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (c->prior != DPMM_PRIOR_MULT) return fail(c, DPMM_EINVAL, who + "the count statistics are those of the Multinomial prior; an NIW ctx has dpmm_batchstats_begin (include/dpmm_hip_batchstats.h)");
    if (mode != DPMM_BATCHSTATS_HARD && mode != DPMM_BATCHSTATS_SOFT) return fail(c, DPMM_EINVAL, who + "mode must be DPMM_BATCHSTATS_HARD or DPMM_BATCHSTATS_SOFT");
    if (!c->predictive) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_predictive_mult first");
    HIPCHK(c, hipSetDevice(c->device));
    c->cs.active = false;
    const int K = c->K, D = c->D;
    const size_t state = sizeof(double) * countstats_acc_doubles(K, D) + sizeof(unsigned long long) * batchstats_count_words(K);
    if (int rc = grow(c, c->d_cs_acc, state, "dpmm_score_points", "accumulators of dpmm_countstats_begin")) return rc;
    if (c->n > 0) {      // one range's floats and partials: sized as dpmm_countstats_accumulate will find them unless the table budget or the store changes in between
        int rstep = 0;
        int64_t P = 0;
        size_t part = 0;
        if (int rc = score_table_slab(c, &rstep, &P)) return rc;
        if (int rc = countstats_range_buffers(c, P, &part)) return rc;
    }
    HIPCHK(c, hipMemsetAsync(c->d_cs_acc, 0, state, c->stream));
    c->cs = AccSession{true, K, mode, use_floor ? 1 : 0, min_logdens, c->pred_gen};
    return DPMM_OK;
}

// t_i of the points p0 .. p0 + nv - 1 into d_cs_tot (one range), for the floor per count
static hipError_t count_totals_range(dpmm_ctx *c, int store, int64_t p0, int64_t nv) {
    CountTotalsArgs t{};
    t.n = nv; t.D = c->D; t.tot = c->d_cs_tot;
    count_points(c, store, p0, t);
    return launch_countstats_totals(t, c->stream);
}

// include/dpmm_hip_countholdout.h: the floor per count of the accumulation just begun
int dpmm_countstats_set_per_count(dpmm_ctx *c, int use, float min_logdens_per_count) {
    return set_second_floor(c, &dpmm_ctx::cs, "dpmm_countstats", "dpmm_countstats_set_per_count", use, min_logdens_per_count,
                            min_logdens_per_count == min_logdens_per_count ? nullptr : "min_logdens_per_count must not be NaN");
}

int dpmm_countstats_accumulate(dpmm_ctx *c, int64_t n_valid) {
    static const char *fn = "dpmm_countstats_accumulate";
    bool empty = false;
    if (int rc = acc_front(c, &dpmm_ctx::cs, "dpmm_countstats_begin", fn, n_valid, nullptr, ACC_COUNTS, &empty)) return rc;
    if (empty) return DPMM_OK;
    const std::string who = std::string(fn) + ": ";
    const int store = count_store(c);
    const int K = c->K, D = c->D;
    size_t part = 0;
    TableWalk w;
    if (int rc = walk_open(c, fn, WALK_MISS_NEVER, &w, [&](int64_t P) -> int {
            if (P >> 31) return fail(c, DPMM_EINVAL, who + RANGE_TOO_LONG);
            return countstats_range_buffers(c, P, &part);
        })) return rc;
    if (c->cs.use2) if (int rc = grow(c, c->d_cs_tot, sizeof(double) * (size_t)w.P, "dpmm_score_points", "totals of dpmm_countstats_accumulate")) return rc;
    c->cs.accumulated = true;
    return walk_ranges(c, w, n_valid, fn, [&](int64_t p0, int64_t, int64_t nv) -> int {
        if (c->cs.use2) if (int rc = table_result(c, fn, count_totals_range(c, store, p0, nv))) return rc;
        CountStatsArgs a{};
        a.table = c->d_score_table; a.stride = w.P; a.rstep = w.rstep; a.n = nv; a.K = K; a.D = D;
        count_points(c, store, p0, a);
        a.soft = c->cs.mode == DPMM_BATCHSTATS_SOFT; a.use_floor = c->cs.floor; a.min_logdens = c->cs.min_logdens;
        a.use_pc = c->cs.use2; a.min_pc = c->cs.min2; a.tot = c->cs.use2 ? c->d_cs_tot.get() : nullptr;
        countstats_chunks(a.n, K, D, store == COUNTSTATS_SPARSE, &a.kgroup, &a.nchunk, &a.chunk, &a.dp);
        if (sizeof(double) * (size_t)a.nchunk * (size_t)a.kgroup * ((size_t)a.dp + 1) > part)
            return fail(c, DPMM_EHIP, who + "internal: more chunks than the partial buffer holds");
        a.ms = c->d_cs_ms;
        a.acc = c->d_cs_acc;
        a.count = reinterpret_cast<unsigned long long *>(c->d_cs_acc + countstats_acc_doubles(K, D));
        a.part = c->d_cs_part;
        a.npart = c->d_cs_part + (size_t)a.nchunk * (size_t)a.kgroup * (size_t)a.dp;
        return table_result(c, fn, launch_countstats_range(a, c->stream));
    });
}

int dpmm_countstats_read(dpmm_ctx *c, const dpmm_countstats_out *o) {
    static const char *fn = "dpmm_countstats_read";
    if (int rc = read_front(c, &dpmm_ctx::cs, "dpmm_countstats_begin", fn, o)) return rc;
    const int K = c->cs.K;
    const size_t D = (size_t)c->D, Kz = (size_t)K;
    hipError_t e = sync_stream(c, c->stream);
    if (e == hipSuccess && o->N) e = hipMemcpy(o->N, c->d_cs_acc, sizeof(double) * Kz, hipMemcpyDeviceToHost);
    if (e == hipSuccess && o->sums) e = hipMemcpy(o->sums, c->d_cs_acc + Kz, sizeof(double) * Kz * D, hipMemcpyDeviceToHost);
    return stats_counters_read(c, fn, e, c->d_cs_acc + countstats_acc_doubles(K, (int)D), K, o->count, o->skipped, o->held_out, o->incomplete);
}

// ---- include/dpmm_hip_recommend.h: the m unseen features of largest next-count probability, range by range (recommend.hip) ---------------
int dpmm_set_recommend(dpmm_ctx *c, const double *theta) {
    static const char *fn = "dpmm_set_recommend";
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (c->prior != DPMM_PRIOR_MULT) return fail(c, DPMM_EINVAL, who + "the next-count probabilities are those of the Multinomial prior: an NIW ctx has dpmm_set_regression");
    if (!theta) return fail(c, DPMM_EINVAL, who + "null table");
    if (!c->predictive) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_predictive_mult first");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t K = (size_t)c->K, Kp = K + (K & 1), D = (size_t)c->D, Dp = (size_t)recommend_pitch(c->D);
    c->rec_gen = 0;      // (a failure below leaves no table in force)
    if (int rc = grow(c, c->d_rec_theta, sizeof(float) * Kp * Dp, fn, "next-count probabilities")) return rc;
    std::vector<float> img(Kp * Dp, 0.f);      // each value rounded to Float32 once; zeros in the pad
    for (size_t k = 0; k < K; ++k)
        for (size_t d = 0; d < D; ++d) img[k * Dp + d] = (float)theta[k * D + d];
    HIPCHK(c, sync_stream(c, c->stream));
    HIPCHK(c, hipMemcpy(c->d_rec_theta, img.data(), sizeof(float) * img.size(), hipMemcpyHostToDevice));
    c->rec_gen = c->pred_gen;
    return DPMM_OK;
}

static int recommend_points(dpmm_ctx *c, int m, int exclude_seen, int32_t *features, float *prob, int64_t ld, int64_t *labels, int64_t *skipped, bool device,
                            const char *fn) {
    if (!c) return tensor_no_ctx(fn);
    c->miss_counted = false;      // (as score_points)
    const std::string who = std::string(fn) + ": ";
    if (c->prior != DPMM_PRIOR_MULT) return fail(c, DPMM_EINVAL, who + "the next-count probabilities are those of the Multinomial prior: an NIW ctx has dpmm_regress_points");
    if (!c->predictive) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_predictive_mult first");
    if (c->rec_gen == 0 || c->rec_gen != c->pred_gen) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_recommend for the predictive parameters in force");
    const int top = std::min(c->D, DPMM_RECOMMEND_MAX_TOP);
    if (m < 1 || m > top) return fail(c, DPMM_EINVAL, who + "m must be in 1.." + std::to_string(top));
    if (ld < m) return fail(c, DPMM_EINVAL, who + "ld < m");
    if (ld >> 40) return fail(c, DPMM_EINVAL, who + "ld out of range");
    HIPCHK(c, hipSetDevice(c->device));
    if (skipped) skipped[0] = 0;
    if (c->n == 0) return DPMM_OK;
    const int store = count_store(c);
    if (!count_store_ready(c, store)) return fail(c, DPMM_ESTATE, who + "needs points and parameters");
    if (!features || !prob) return fail(c, DPMM_EINVAL, who + (features ? "prob is null" : "features is null"));
    // the rows: in the caller's device memory ld words apart; staged (host variant) dense, m apart
    const size_t rb = 4 * (size_t)m, pb = 4 * (size_t)ld;      // (4-byte words both)
    OutStage<3> out{{{features, "d_features", 4, rb, pb}, {prob, "d_prob", 4, rb, pb}, {labels, "d_labels", 8, sizeof(int64_t)}}, device};
    if (int rc = out.check(c, fn, (uint64_t)c->n)) return rc;
    TableWalk w;
    if (int rc = walk_open(c, fn, WALK_MISS_NEVER, &w)) return rc;
    if (int rc = skip_open(c, c->d_rec_skip, w.P, fn, "counts of the recommendation pass")) return rc;
    if (int rc = out.open(c, w.P)) return rc;
    if (int rc = walk_ranges(c, w, c->n, fn, [&](int64_t p0, int64_t np, int64_t) {
            RecommendArgs a{};
            a.table = c->d_score_table; a.stride = w.P; a.rstep = w.rstep; a.n = np; a.K = c->K; a.Kp = c->K + (c->K & 1); a.D = c->D; a.Dp = recommend_pitch(c->D);
            count_points(c, store, p0, a);
            a.theta = c->d_rec_theta; a.m = m; a.exclude = exclude_seen ? 1 : 0;
            a.features = out.at<int32_t>(0, p0); a.prob = out.at<float>(1, p0); a.ld = device ? ld : m; a.labels = out.at<int64_t>(2, p0); a.skip = c->d_rec_skip;
            hipError_t e = launch_recommend_range(a, c->stream);
            if (e == hipSuccess && !device) e = out.flush(c, p0, (size_t)np);
            return e;
        })) return rc;
    return skip_close(c, c->d_rec_skip, w.P, skipped);
}

int dpmm_recommend_points(dpmm_ctx *c, int m, int exclude_seen, int32_t *features, float *prob, int64_t ld, int64_t *labels, int64_t *skipped) {
    return recommend_points(c, m, exclude_seen, features, prob, ld, labels, skipped, false, "dpmm_recommend_points");
}
int dpmm_recommend_points_device(dpmm_ctx *c, int m, int exclude_seen, int32_t *d_features, float *d_prob, int64_t ld, int64_t *d_labels, int64_t *skipped) {
    return recommend_points(c, m, exclude_seen, d_features, d_prob, ld, d_labels, skipped, true, "dpmm_recommend_points_device");
}

// ---- include/dpmm_hip_count_explain.h: the features that put a count point out, range by range (count_explain.hip) ----------------------
int dpmm_set_count_explain(dpmm_ctx *c, const double *log_theta, const double *log1m_theta, const int32_t *order) {
    static const char *fn = "dpmm_set_count_explain";
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (c->prior != DPMM_PRIOR_MULT) return fail(c, DPMM_EINVAL, who + "the binomial law of a feature is that of the Multinomial prior: an NIW ctx has dpmm_explain_points");
    if (!log_theta || !log1m_theta || !order) return fail(c, DPMM_EINVAL, who + "null table");
    if (!c->predictive) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_predictive_mult first");
    const size_t K = (size_t)c->K, D = (size_t)c->D;
    // the kernel indexes the tables with what `order` holds and ends its walk on what the order promises: both are checked here
    std::vector<char> seen(D);
    for (size_t k = 0; k < K; ++k) {
        std::fill(seen.begin(), seen.end(), 0);
        for (size_t j = 0; j < D; ++j) {
            const double a = log_theta[k * D + j], b = log1m_theta[k * D + j];
            if (!(a <= 0.) || !(b <= 0.)) return fail(c, DPMM_EINVAL, who + "a logarithm of a probability is above 0 or NaN");
            const int32_t d = order[k * D + j];
            if (d < 0 || (size_t)d >= D || seen[(size_t)d]) return fail(c, DPMM_EINVAL, who + "order is no permutation of the features");
            seen[(size_t)d] = 1;
            if (j > 0) {
                const int32_t p = order[k * D + j - 1];
                const double lp = log1m_theta[k * D + (size_t)p], ld = log1m_theta[k * D + (size_t)d];
                if (!(lp < ld || (lp == ld && p < d))) return fail(c, DPMM_EINVAL, who + "order does not follow log1m_theta (non-decreasing, ties to the lower index)");
            }
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    c->cex_gen = 0;      // (a failure below leaves no table in force)
    if (int rc = grow(c, c->d_cex_log, sizeof(double) * 2 * K * D, fn, "logarithms of the feature probabilities")) return rc;
    if (int rc = grow(c, c->d_cex_order, sizeof(int32_t) * K * D, fn, "order of the feature probabilities")) return rc;
    HIPCHK(c, sync_stream(c, c->stream));
    HIPCHK(c, hipMemcpy(c->d_cex_log, log_theta, sizeof(double) * K * D, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_cex_log + K * D, log1m_theta, sizeof(double) * K * D, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_cex_order, order, sizeof(int32_t) * K * D, hipMemcpyHostToDevice));
    c->cex_gen = c->pred_gen;
    return DPMM_OK;
}

static int count_explain_points(dpmm_ctx *c, const dpmm_count_explain_out *o, bool device, const char *fn) {
    if (!c) return tensor_no_ctx(fn);
    c->miss_counted = false;      // (as score_points)
    const std::string who = std::string(fn) + ": ";
    if (c->prior != DPMM_PRIOR_MULT) return fail(c, DPMM_EINVAL, who + "the binomial law of a feature is that of the Multinomial prior: an NIW ctx has dpmm_explain_points");
    if (!o) return fail(c, DPMM_EINVAL, who + "null out");
    if (!c->predictive) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_predictive_mult first");
    if (c->cex_gen == 0 || c->cex_gen != c->pred_gen) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_count_explain for the predictive parameters in force");
    const int cap = std::min(c->D, DPMM_COUNT_EXPLAIN_MAX_TOP), top = o->top;
    const int64_t ld = o->ld;
    if (top < 1 || top > cap) return fail(c, DPMM_EINVAL, who + "top must be in 1.." + std::to_string(cap));
    if (o->side < DPMM_COUNT_EXPLAIN_BOTH || o->side > DPMM_COUNT_EXPLAIN_UNDER) return fail(c, DPMM_EINVAL, who + "side must be DPMM_COUNT_EXPLAIN_BOTH, _OVER or _UNDER");
    if (ld < top) return fail(c, DPMM_EINVAL, who + "ld < top");
    if (ld >> 40) return fail(c, DPMM_EINVAL, who + "ld out of range");
    HIPCHK(c, hipSetDevice(c->device));
    if (o->skipped) o->skipped[0] = 0;
    if (o->incomplete) o->incomplete[0] = 0;
    if (c->n == 0) return DPMM_OK;
    const int store = count_store(c);
    if (!count_store_ready(c, store)) return fail(c, DPMM_ESTATE, who + "needs points and parameters");
    // the rows: in the caller's device memory ld words apart; staged (host variant) dense, top apart
    const size_t rb = sizeof(float) * (size_t)top, pb = sizeof(float) * (size_t)ld;      // (the five arrays have 4-byte words)
    OutStage<7> out{{{o->features, "d_features", 4, rb, pb}, {o->count, "d_count", 4, rb, pb}, {o->expected, "d_expected", 4, rb, pb}, {o->residual, "d_residual", 4, rb, pb},
                     {o->feature_tail, "d_feature_tail", 4, rb, pb}, {o->labels, "d_labels", 8, sizeof(int64_t)}, {o->total, "d_total", 8, sizeof(double)}}, device};
    for (int i = 0; i < 5; ++i)
        if (!out.col[i].dst) return fail(c, DPMM_EINVAL, who + (out.col[i].name + 2) + " is null");      // (the field's name: without the d_)
    if (int rc = out.check(c, fn, (uint64_t)c->n)) return rc;
    TableWalk w;
    if (int rc = walk_open(c, fn, WALK_MISS_NEVER, &w)) return rc;
    if (int rc = skip_open(c, c->d_cex_skip, w.P, fn, "counts of the skipped points")) return rc;
    if (int rc = skip_open(c, c->d_cex_inc, w.P, fn, "counts of the incomplete points")) return rc;
    if (int rc = grow(c, c->d_cex_tot, sizeof(double) * (size_t)w.P, fn, "totals of the points")) return rc;
    if (int rc = grow(c, c->d_cex_lab, sizeof(int32_t) * (size_t)w.P, fn, "labels of the points")) return rc;
    if (int rc = out.open(c, w.P)) return rc;
    const size_t KD = (size_t)c->K * (size_t)c->D;
    if (int rc = walk_ranges(c, w, c->n, fn, [&](int64_t p0, int64_t np, int64_t) {
            CountExplainArgs a{};
            a.table = c->d_score_table; a.stride = w.P; a.rstep = w.rstep; a.n = np; a.K = c->K; a.D = c->D;
            count_points(c, store, p0, a);
            a.lth = c->d_cex_log; a.l1m = c->d_cex_log + KD; a.order = c->d_cex_order; a.top = top; a.side = o->side;
            a.features = out.at<int32_t>(0, p0); a.count = out.at<float>(1, p0); a.expected = out.at<float>(2, p0); a.residual = out.at<float>(3, p0);
            a.feature_tail = out.at<float>(4, p0); a.ld = device ? ld : top; a.labels = out.at<int64_t>(5, p0); a.total = out.at<double>(6, p0);
            a.skip = c->d_cex_skip; a.incomplete = c->d_cex_inc; a.tot = c->d_cex_tot; a.lab = c->d_cex_lab;
            hipError_t e = launch_count_explain_range(a, c->stream);
            if (e == hipSuccess && !device) e = out.flush(c, p0, (size_t)np);
            return e;
        })) return rc;
    if (int rc = skip_close(c, c->d_cex_skip, w.P, o->skipped)) return rc;
    return skip_close(c, c->d_cex_inc, w.P, o->incomplete);
}

int dpmm_count_explain_points(dpmm_ctx *c, const dpmm_count_explain_out *out) { return count_explain_points(c, out, false, "dpmm_count_explain_points"); }
int dpmm_count_explain_points_device(dpmm_ctx *c, const dpmm_count_explain_out *out) { return count_explain_points(c, out, true, "dpmm_count_explain_points_device"); }

// ---- include/dpmm_hip_countholdout.h: the held-out points of a batch of count data, compacted into the caller's device memory (holdout.hip)
// kind of a destination: 0 count only, 1 rows of Float32 (dense stores), 2 compressed sparse columns
static int countholdout_kind(const dpmm_countholdout_dst &d) { return d.cap <= 0 ? 0 : d.colptr ? 2 : 1; }
static int countholdout_check_dst(dpmm_ctx *c, const char *fn, const dpmm_countholdout_dst &d) {
    if (d.cap <= 0) return DPMM_OK;
    if (int rc = check_device_extent(c, fn, "dst_index", d.index, (uint64_t)d.cap * sizeof(int64_t), sizeof(int64_t))) return rc;
    if (countholdout_kind(d) == 1) return check_device_extent(c, fn, "dst_points", d.points, (uint64_t)d.cap * (uint64_t)c->D * sizeof(float), sizeof(float));
    if (int rc = check_device_extent(c, fn, "dst_colptr", d.colptr, ((uint64_t)d.cap + 1) * sizeof(int64_t), sizeof(int64_t))) return rc;
    if (int rc = check_device_extent(c, fn, "dst_rowval", d.rowval, (uint64_t)d.entry_cap * sizeof(int32_t), sizeof(int32_t))) return rc;
    return check_device_extent(c, fn, "dst_val", d.val, (uint64_t)d.entry_cap * sizeof(float), sizeof(float));
}

int dpmm_countholdout_begin(dpmm_ctx *c, int use_floor, float min_logdens, int use_per_count, float min_logdens_per_count, const dpmm_countholdout_dst *dst) {
    static const char *fn = "dpmm_countholdout_begin";
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (c->prior != DPMM_PRIOR_MULT) return fail(c, DPMM_EINVAL, who + "held-out count points are collected under the Multinomial prior; an NIW ctx has dpmm_holdout_begin (include/dpmm_hip_holdout.h)");
    if (!use_floor && !use_per_count) return fail(c, DPMM_EINVAL, who + "needs a floor: use_floor or use_per_count");
    if (use_per_count && min_logdens_per_count != min_logdens_per_count) return fail(c, DPMM_EINVAL, who + "min_logdens_per_count must not be NaN");
    dpmm_countholdout_dst d = {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
    if (dst) d = *dst;
    if (d.cap < 0 || (d.cap >> 40) || d.entry_cap < 0 || (d.entry_cap >> 48)) return fail(c, DPMM_EINVAL, who + "cap must be in 0..2^40 - 1 and entry_cap in 0..2^48 - 1");
    if (d.cap > 0 && d.points && d.colptr) return fail(c, DPMM_EINVAL, who + "the destination is either dst_points (dense stores) or dst_colptr / dst_rowval / dst_val (sparse store), not both");
    if (d.cap > 0 && !d.points && !d.colptr) return fail(c, DPMM_EINVAL, who + "cap > 0 needs a destination: dst_points or dst_colptr");
    if (!c->predictive) return fail(c, DPMM_ESTATE, who + "needs dpmm_set_predictive_mult first");
    HIPCHK(c, hipSetDevice(c->device));
    c->ch.active = false;
    if (int rc = countholdout_check_dst(c, fn, d)) return rc;
    if (int rc = grow(c, c->d_ch_state, sizeof(unsigned long long) * COUNTHOLDOUT_STATE, "dpmm_score_points", "counters of dpmm_countholdout_begin")) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_ch_state, 0, sizeof(unsigned long long) * COUNTHOLDOUT_STATE, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_ch_state + 5, 0xFF, sizeof(unsigned long long) * 2, c->stream));      // stored, stored entries: COUNTHOLDOUT_UNSET
    if (countholdout_kind(d) == 2) HIPCHK(c, hipMemsetAsync(d.colptr, 0, sizeof(int64_t), c->stream));    // slot 0
    c->ch = AccSession{true, c->K, 0, use_floor ? 1 : 0, min_logdens, c->pred_gen, use_per_count ? 1 : 0, use_per_count ? min_logdens_per_count : 0.f};
    c->ch_dst = d;
    return DPMM_OK;
}

int dpmm_countholdout_accumulate(dpmm_ctx *c, int64_t lo, int64_t n_valid) {
    static const char *fn = "dpmm_countholdout_accumulate";
    bool empty = false;
    if (int rc = acc_front(c, &dpmm_ctx::ch, "dpmm_countholdout_begin", fn, n_valid, &lo, ACC_COUNTS, &empty)) return rc;
    if (empty) return DPMM_OK;
    const std::string who = std::string(fn) + ": ";
    const int store = count_store(c);
    const int kind = countholdout_kind(c->ch_dst);
    if (kind != 0 && (kind == 2) != (store == COUNTSTATS_SPARSE))
        return fail(c, DPMM_ESTATE, who + (store == COUNTSTATS_SPARSE ? "the sparse store is live and dpmm_countholdout_begin was given the dense destination dst_points"
                                                                      : "a dense store is live and dpmm_countholdout_begin was given the sparse destination dst_colptr"));
    if (int rc = countholdout_check_dst(c, fn, c->ch_dst)) return rc;      // (the caller may have freed it since the begin)
    TableWalk w;
    if (int rc = walk_open(c, fn, WALK_MISS_NEVER, &w, [&](int64_t P) -> int {
            if (P >> 31) return fail(c, DPMM_EINVAL, who + RANGE_TOO_LONG);
            return holdout_range_buffers(c, P, true);
        })) return rc;
    if (c->ch.use2) if (int rc = grow(c, c->d_cs_tot, sizeof(double) * (size_t)w.P, "dpmm_score_points", "totals of dpmm_countholdout_accumulate")) return rc;
    return walk_ranges(c, w, n_valid, fn, [&](int64_t p0, int64_t, int64_t nv) -> int {
        if (c->ch.use2) if (int rc = table_result(c, fn, count_totals_range(c, store, p0, nv))) return rc;
        CountHoldoutArgs a{};
        a.table = c->d_score_table; a.stride = w.P; a.rstep = w.rstep; a.n = nv; a.K = c->K; a.D = c->D;
        count_points(c, store, p0, a);
        a.use_floor = c->ch.floor; a.min_logdens = c->ch.min_logdens;
        a.use_pc = c->ch.use2; a.min_pc = c->ch.min2; a.tot = c->ch.use2 ? c->d_cs_tot.get() : nullptr;
        a.index0 = lo + p0;
        a.ballot = c->d_ho_ballot; a.wgcount = c->d_ho_count; a.wgent = c->d_ch_ent; a.wgoff = c->d_ho_off; a.wgeoff = c->d_ch_eoff; a.state = c->d_ch_state;
        a.dst_points = c->ch_dst.points; a.dst_colptr = c->ch_dst.colptr; a.dst_rowval = c->ch_dst.rowval; a.dst_val = c->ch_dst.val; a.dst_index = c->ch_dst.index;
        a.cap = c->ch_dst.cap; a.entry_cap = kind == 2 ? c->ch_dst.entry_cap : 0;
        return table_result(c, fn, launch_countholdout_range(a, c->stream));
    });
}

int dpmm_countholdout_read(dpmm_ctx *c, const dpmm_countholdout_out *o) {
    static const char *fn = "dpmm_countholdout_read";
    if (int rc = read_front(c, &dpmm_ctx::ch, "dpmm_countholdout_begin", fn, o)) return rc;
    unsigned long long h[COUNTHOLDOUT_STATE] = {0, 0, 0, 0, 0, 0, 0, 0};
    hipError_t e = sync_stream(c, c->stream);
    if (e == hipSuccess) e = hipMemcpy(h, c->d_ch_state, sizeof(h), hipMemcpyDeviceToHost);
    if (int rc = table_result(c, fn, e)) return rc;
    const int kind = countholdout_kind(c->ch_dst);
    // dense stores: an entry is a feature; sparse store: the one workgroup that met a cap wrote [5] and [6], else everything fitted
    const int64_t total = (int64_t)h[0], entries = c->x_sparse ? (int64_t)h[4] : total * c->D;
    int64_t stored = 0, stored_entries = 0;
    if (kind == 1) { stored = std::min<int64_t>(total, c->ch_dst.cap); stored_entries = stored * c->D; }
    else if (kind == 2) { stored = h[5] == COUNTHOLDOUT_UNSET ? total : (int64_t)h[5]; stored_entries = h[5] == COUNTHOLDOUT_UNSET ? (int64_t)h[4] : (int64_t)h[6]; }
    if (o->total) o->total[0] = total;
    if (o->total_entries) o->total_entries[0] = entries;
    if (o->stored) o->stored[0] = stored;
    if (o->stored_entries) o->stored_entries[0] = stored_entries;
    if (o->skipped) o->skipped[0] = (int64_t)h[1];
    if (o->incomplete) o->incomplete[0] = (int64_t)h[2];
    if (o->scored) o->scored[0] = (int64_t)h[3];
    return DPMM_OK;
}

// ---- include/dpmm_hip_trace.h: label samples kept on the device, their contingency tables and the per-point confidence (trace.hip) ----------
static uint16_t *trace_row(dpmm_ctx *c, int slot) { return c->d_trace + (size_t)slot * (size_t)c->trace_nvec * 8; }
// a slot a call names: inside the trace (DPMM_EINVAL) and recorded (DPMM_ESTATE)
static int trace_slot_ok(dpmm_ctx *c, const std::string &who, int slot) {
    if (slot < 0 || slot >= c->trace_slots) return fail(c, DPMM_EINVAL, who + "slot " + std::to_string(slot) + " is outside 0.." + std::to_string(c->trace_slots - 1));
    if (c->trace_K[slot] == 0) return fail(c, DPMM_ESTATE, who + "slot " + std::to_string(slot) + " was never recorded");
    return DPMM_OK;
}

int dpmm_trace_close(dpmm_ctx *c) {
    static const char *fn = "dpmm_trace_close";
    if (!c) return tensor_no_ctx(fn);
    if (!c->d_trace) return DPMM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_stream(c, c->stream));
    c->d_trace.reset();
    c->trace_slots = 0; c->trace_nvec = 0; c->trace_K.clear();
    return DPMM_OK;
}

int dpmm_trace_open(dpmm_ctx *c, int slots) {
    static const char *fn = "dpmm_trace_open";
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (slots < 1 || slots > DPMM_TRACE_MAX_SLOTS) return fail(c, DPMM_EINVAL, who + "slots must be in 1.." + std::to_string(DPMM_TRACE_MAX_SLOTS));
    if (int rc = dpmm_trace_close(c)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t nvec = (c->n + 7) / 8;                           // a row: n ids of 2 bytes, padded to 16 bytes
    const size_t bytes = std::max<size_t>(16, (size_t)slots * (size_t)nvec * 16);
    if (int rc = regrow(c, c->d_trace, bytes, fn, "trace")) return rc;      // (dpmm_trace_close above waited for the stream)
    c->trace_slots = slots; c->trace_nvec = nvec; c->trace_K.assign((size_t)slots, 0);
    return DPMM_OK;
}

int dpmm_trace_record(dpmm_ctx *c, int slot, int K) {
    static const char *fn = "dpmm_trace_record";
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (!c->d_trace) return fail(c, DPMM_ESTATE, who + "needs dpmm_trace_open first");
    if (!c->have_labels) return fail(c, DPMM_ESTATE, who + "labels not initialised");
    if (slot < 0 || slot >= c->trace_slots) return fail(c, DPMM_EINVAL, who + "slot " + std::to_string(slot) + " is outside 0.." + std::to_string(c->trace_slots - 1));
    if (K < 1 || K > DPMM_MAX_CLUSTERS) return fail(c, DPMM_EINVAL, who + "K must be in 1..DPMM_MAX_CLUSTERS");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_trace_record(c->dbins, c->n, trace_row(c, slot), c->trace_nvec, c->stream));
    c->trace_K[slot] = K;
    return DPMM_OK;
}

int dpmm_trace_tables(dpmm_ctx *c, const int32_t *pairs, int npairs, int64_t *counts) {
    static const char *fn = "dpmm_trace_tables";
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (npairs < 0 || (npairs > 0 && (!pairs || !counts))) return fail(c, DPMM_EINVAL, who + "npairs < 0 or a null pointer");
    if (!c->d_trace) return fail(c, DPMM_ESTATE, who + "needs dpmm_trace_open first");
    std::vector<size_t> off((size_t)npairs + 1, 0);
    for (int p = 0; p < npairs; ++p) {
        if (int rc = trace_slot_ok(c, who, pairs[2 * p])) return rc;
        if (int rc = trace_slot_ok(c, who, pairs[2 * p + 1])) return rc;
        off[p + 1] = off[p] + (size_t)c->trace_K[pairs[2 * p]] * (size_t)c->trace_K[pairs[2 * p + 1]];
    }
    const size_t total = off[npairs];
    if (total == 0) return DPMM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0) { memset(counts, 0, sizeof(int64_t) * total); return DPMM_OK; }
    if (int rc = grow(c, c->d_trace_counts, sizeof(unsigned long long) * total, fn, "tables")) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_trace_counts, 0, sizeof(unsigned long long) * total, c->stream));
    // pairs by row slot (stable: a row's pairs keep their order), then consecutive pairs of a row into groups within the LDS budget
    std::vector<int> order((size_t)npairs);
    for (int p = 0; p < npairs; ++p) order[p] = p;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return pairs[2 * a] < pairs[2 * b]; });
    std::vector<TraceGroup> groups;
    std::vector<TracePair> tp;
    std::vector<int> big;
    int max_cells = 0;
    for (int q = 0; q < npairs; ++q) {
        const int p = order[q], s = pairs[2 * p], t = pairs[2 * p + 1];
        const int Ks = c->trace_K[s], Kt = c->trace_K[t], cells = Ks * Kt;      // (at most 1024 * 1024)
        if (cells > TRACE_LDS_CELLS) { big.push_back(p); continue; }
        if (groups.empty() || groups.back().zs != trace_row(c, s) || groups.back().cells + cells > TRACE_LDS_CELLS) {
            TraceGroup g{};
            g.zs = trace_row(c, s); g.Ks = Ks; g.pair0 = (int)tp.size(); g.npairs = 0; g.cells = 0;
            groups.push_back(g);
        }
        TraceGroup &g = groups.back();
        TracePair e{};
        e.zt = trace_row(c, t); e.Kt = Kt; e.cell0 = (unsigned)g.cells; e.out = c->d_trace_counts + off[p];
        tp.push_back(e);
        g.npairs += 1; g.cells += cells;
        max_cells = std::max(max_cells, g.cells);
    }
    if (!groups.empty()) {
        const size_t gb = (sizeof(TraceGroup) * groups.size() + 15) & ~(size_t)15, pb = sizeof(TracePair) * tp.size();
        if (int rc = grow(c, c->d_trace_desc, gb + pb, fn, "pair lists")) return rc;
        HIPCHK(c, hipMemcpy(c->d_trace_desc, groups.data(), sizeof(TraceGroup) * groups.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_trace_desc + gb, tp.data(), pb, hipMemcpyHostToDevice));
        HIPCHK(c, launch_trace_tables(reinterpret_cast<const TraceGroup *>(c->d_trace_desc.get()), (int)groups.size(),
                                      reinterpret_cast<const TracePair *>(c->d_trace_desc + gb), max_cells, c->trace_nvec, c->stream));
    }
    for (int p : big) {
        const int s = pairs[2 * p], t = pairs[2 * p + 1];
        HIPCHK(c, launch_trace_pair_global(trace_row(c, s), trace_row(c, t), c->trace_K[s], c->trace_K[t], c->trace_nvec, c->d_trace_counts + off[p], c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(counts, c->d_trace_counts, sizeof(unsigned long long) * total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, sync_stream(c, c->stream));
    return DPMM_OK;
}

int dpmm_trace_confidence(dpmm_ctx *c, int anchor, const int32_t *slots, int nslots, const float *ratio, float *out_host, void *out_device) {
    static const char *fn = "dpmm_trace_confidence";
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (nslots < 1 || nslots > DPMM_TRACE_MAX_SLOTS) return fail(c, DPMM_EINVAL, who + "nslots must be in 1.." + std::to_string(DPMM_TRACE_MAX_SLOTS));
    if (!slots || !ratio) return fail(c, DPMM_EINVAL, who + "slots or ratio is null");
    if (!out_host && !out_device) return fail(c, DPMM_EINVAL, who + "no output given");
    if (!c->d_trace) return fail(c, DPMM_ESTATE, who + "needs dpmm_trace_open first");
    if (int rc = trace_slot_ok(c, who, anchor)) return rc;
    const int Ka = c->trace_K[anchor];
    std::vector<TraceConfSlot> cs((size_t)nslots);
    uint64_t total = 0;
    for (int j = 0; j < nslots; ++j) {
        if (int rc = trace_slot_ok(c, who, slots[j])) return rc;
        cs[j].z = trace_row(c, slots[j]); cs[j].K = c->trace_K[slots[j]]; cs[j].off = (unsigned)total;
        total += (uint64_t)Ka * (uint64_t)cs[j].K;
        if (total >> 32) return fail(c, DPMM_EINVAL, who + "the ratio tables hold 2^32 entries or more");
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0) return DPMM_OK;
    if (out_device) if (int rc = check_device_extent(c, fn, "out_device", out_device, sizeof(float) * (uint64_t)c->n, sizeof(float))) return rc;
    if (int rc = grow(c, c->d_trace_ratio, sizeof(float) * (size_t)total, fn, "ratio tables")) return rc;
    if (int rc = grow(c, c->d_trace_desc, sizeof(TraceConfSlot) * cs.size(), fn, "slot list")) return rc;
    float *target = static_cast<float *>(out_device);
    if (!target) {
        if (int rc = grow(c, c->d_trace_conf, sizeof(float) * (size_t)c->n, fn, "result")) return rc;
        target = c->d_trace_conf;
    }
    HIPCHK(c, hipMemcpy(c->d_trace_ratio, ratio, sizeof(float) * (size_t)total, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_trace_desc, cs.data(), sizeof(TraceConfSlot) * cs.size(), hipMemcpyHostToDevice));
    HIPCHK(c, launch_trace_confidence(trace_row(c, anchor), Ka, reinterpret_cast<const TraceConfSlot *>(c->d_trace_desc.get()), nslots, c->d_trace_ratio, c->n,
                                      c->trace_nvec, target, c->stream));
    if (out_host) HIPCHK(c, hipMemcpyAsync(out_host, target, sizeof(float) * (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, sync_stream(c, c->stream));
    return DPMM_OK;
}

int dpmm_trace_read(dpmm_ctx *c, int slot, int64_t *labels_host, void *labels_device) {
    static const char *fn = "dpmm_trace_read";
    if (!c) return tensor_no_ctx(fn);
    const std::string who = std::string(fn) + ": ";
    if (!labels_host && !labels_device) return fail(c, DPMM_EINVAL, who + "no output given");
    if (!c->d_trace) return fail(c, DPMM_ESTATE, who + "needs dpmm_trace_open first");
    if (int rc = trace_slot_ok(c, who, slot)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0) return DPMM_OK;
    if (labels_device) if (int rc = check_device_extent(c, fn, "labels_device", labels_device, sizeof(int64_t) * (uint64_t)c->n, sizeof(int64_t))) return rc;
    DevBuf<int64_t> tmp;
    int64_t *target = static_cast<int64_t *>(labels_device);
    if (!target) {
        HIPCHK(c, tmp.alloc(sizeof(int64_t) * (size_t)c->n));
        target = tmp;
    }
    hipError_t e = launch_trace_read(trace_row(c, slot), c->n, target, c->stream);
    if (e == hipSuccess && labels_host) e = hipMemcpyAsync(labels_host, target, sizeof(int64_t) * (size_t)c->n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = sync_stream(c, c->stream);
    if (e != hipSuccess) { c->err = who + hipGetErrorString(e); return DPMM_EHIP; }
    return DPMM_OK;
}

// ---- include/dpmm_hip_sample.h: drawing points from a fitted model (sample.hip) -------------------------------------------------------
int dpmm_set_sampler_niw(dpmm_ctx *c, int K, const float *m, const float *A, const float *df) {
    static const std::string who = "dpmm_set_sampler_niw: ";
    if (!c) return tensor_no_ctx("dpmm_set_sampler_niw");
    if (c->prior != DPMM_PRIOR_NIW) return fail(c, DPMM_EINVAL, who + "the context is not an NIW one");
    if (K < 1 || K > DPMM_MAX_CLUSTERS) return fail(c, DPMM_EINVAL, who + "K must be in 1..DPMM_MAX_CLUSTERS");
    if (!m || !A || !df) return fail(c, DPMM_EINVAL, who + "m, A or df is null");
    const int D = c->D;
    for (int k = 0; k < K; ++k)
        if (!(df[k] > 0.f) || !std::isfinite(df[k])) return fail(c, DPMM_EINVAL, who + "df[" + std::to_string(k) + "] is not a positive finite number");
    // the kernel reads the factor transposed (its lanes run along the rows of A), with exact zeros below the diagonal
    std::vector<float> At((size_t)K * D * D, 0.f);
    for (int k = 0; k < K; ++k)
        for (int a = 0; a < D; ++a)
            for (int b = a; b < D; ++b) At[((size_t)k * D + b) * D + a] = A[((size_t)k * D + a) * D + b];
    HIPCHK(c, hipSetDevice(c->device));
    c->sm_K = 0;
    if (int rc = sampler_table(c, c->d_sm_m, m, sizeof(float) * (size_t)K * D)) return rc;
    if (int rc = sampler_table(c, c->d_sm_At, At.data(), sizeof(float) * At.size())) return rc;
    if (int rc = sampler_table(c, c->d_sm_df, df, sizeof(float) * (size_t)K)) return rc;
    c->sm_K = K;
    return DPMM_OK;
}

int dpmm_set_sampler_mult(dpmm_ctx *c, int K, const uint32_t *thr, const int32_t *alias) {
    static const std::string who = "dpmm_set_sampler_mult: ";
    if (!c) return tensor_no_ctx("dpmm_set_sampler_mult");
    if (c->prior != DPMM_PRIOR_MULT) return fail(c, DPMM_EINVAL, who + "the context is not a Multinomial one");
    if (K < 1 || K > DPMM_MAX_CLUSTERS) return fail(c, DPMM_EINVAL, who + "K must be in 1..DPMM_MAX_CLUSTERS");
    if (!thr || !alias) return fail(c, DPMM_EINVAL, who + "thr or alias is null");
    const size_t cnt = (size_t)K * c->D;
    for (size_t e = 0; e < cnt; ++e)
        if (alias[e] < 0 || alias[e] >= c->D) return fail(c, DPMM_EINVAL, who + "alias[" + std::to_string(e) + "] is outside [0, D)");
    HIPCHK(c, hipSetDevice(c->device));
    c->sm_K = 0;
    if (int rc = sampler_table(c, c->d_sm_thr, thr, sizeof(uint32_t) * cnt)) return rc;
    if (int rc = sampler_table(c, c->d_sm_alias, alias, sizeof(int32_t) * cnt)) return rc;
    c->sm_K = K;
    return DPMM_OK;
}

int dpmm_sample_points_device(dpmm_ctx *c, const dpmm_sample_request *q) {
    static const char *fn = "dpmm_sample_points_device";
    const std::string who = std::string(fn) + ": ";
    if (!c) return tensor_no_ctx(fn);
    if (!q) return fail(c, DPMM_EINVAL, who + "the request is null");
    if (c->sm_K < 1) return fail(c, DPMM_ESTATE, who + "no sampler set (dpmm_set_sampler_niw / _mult)");
    const int K = c->sm_K, D = c->D;
    const bool mult = c->prior == DPMM_PRIOR_MULT;
    const bool sparse = q->colptr != nullptr;
    if (q->n < 0 || q->n > c->n) return fail(c, DPMM_EINVAL, who + "n must be in 0..n_local (" + std::to_string((long long)c->n) + ")");
    if (q->i0 < 0 || q->i0 > INT64_MAX - q->n) return fail(c, DPMM_EINVAL, who + "i0 out of range");
    if (!q->cluster_start) return fail(c, DPMM_EINVAL, who + "cluster_start is null");
    for (int k = 0; k < K; ++k)
        if (q->cluster_start[k] < 0 || q->cluster_start[k + 1] < q->cluster_start[k]) return fail(c, DPMM_EINVAL, who + "cluster_start is negative or decreases");
    if (q->n > 0 && (q->i0 < q->cluster_start[0] || q->i0 + q->n > q->cluster_start[K]))
        return fail(c, DPMM_EINVAL, who + "[i0, i0 + n) is not inside [cluster_start[0], cluster_start[K])");
    if (mult) {
        if (q->trials < 1) return fail(c, DPMM_EINVAL, who + "trials must be at least 1 for a Multinomial context");
        if (sparse && q->trials > DPMM_SAMPLE_MAX_TRIALS_SPARSE) return fail(c, DPMM_EINVAL, who + "trials > DPMM_SAMPLE_MAX_TRIALS_SPARSE");
        if (q->trials > DPMM_SAMPLE_MAX_TRIALS_DENSE) return fail(c, DPMM_EINVAL, who + "trials > DPMM_SAMPLE_MAX_TRIALS_DENSE");
    } else {
        if (q->trials != 0) return fail(c, DPMM_EINVAL, who + "trials must be 0 for an NIW context");
        if (sparse) return fail(c, DPMM_EINVAL, who + "sparse output is for Multinomial contexts");
    }
    const bool fill = sparse && (q->rowval || q->nzval);
    if (sparse) {
        if (q->x) return fail(c, DPMM_EINVAL, who + "x and colptr are both set");
        if (D > DPMM_MAX_DIM_MULT_SPARSE) return fail(c, DPMM_ELIMIT, who + "D > DPMM_MAX_DIM_MULT_SPARSE");
        if (q->nnz0 < 0 || (q->nnz0 >> 58)) return fail(c, DPMM_EINVAL, who + "nnz0 out of range");
        if (fill && (q->nnz_extent < 0 || (q->nnz_extent >> 58))) return fail(c, DPMM_EINVAL, who + "nnz_extent out of range");
        if (!fill && !q->nnz_out) return fail(c, DPMM_EINVAL, who + "nnz_out is null");
    } else {
        if (q->ld < D || (q->ld >> 40)) return fail(c, DPMM_EINVAL, who + "ld < D or out of range");
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (q->n == 0) {
        if (sparse && !fill) {
            if (int rc = check_device_extent(c, fn, "colptr", q->colptr, sizeof(int64_t), sizeof(int64_t))) return rc;
            HIPCHK(c, hipMemcpy(q->colptr, &q->nnz0, sizeof(int64_t), hipMemcpyHostToDevice));
            *q->nnz_out = 0;
        }
        return DPMM_OK;
    }
    const uint64_t n = (uint64_t)q->n;
    if (sparse) {
        if (int rc = check_device_extent(c, fn, "colptr", q->colptr, sizeof(int64_t) * (n + 1), sizeof(int64_t))) return rc;
        if (fill) {
            if (int rc = check_device_extent(c, fn, "rowval", q->rowval, sizeof(int64_t) * (uint64_t)q->nnz_extent, sizeof(int64_t))) return rc;
            if (int rc = check_device_extent(c, fn, "nzval", q->nzval, sizeof(float) * (uint64_t)q->nnz_extent, sizeof(float))) return rc;
            if (q->nnz_extent > 0 && (!q->rowval || !q->nzval)) return fail(c, DPMM_EINVAL, who + "rowval or nzval is null");
        }
    } else {
        if (int rc = check_device_extent(c, fn, "x", q->x, sizeof(float) * ((n - 1) * (uint64_t)q->ld + (uint64_t)D), sizeof(float))) return rc;
    }
    if (q->labels) if (int rc = check_device_extent(c, fn, "labels", q->labels, sizeof(int64_t) * n, sizeof(int64_t))) return rc;
    // cluster (and, NIW, 64-point tile) starts relative to the call
    std::vector<int64_t> cs((size_t)K + 1);
    std::vector<int32_t> ts((size_t)K + 1);
    int64_t tiles = 0;
    for (int k = 0; k <= K; ++k) {
        cs[k] = std::min<int64_t>(std::max<int64_t>(q->cluster_start[k] - q->i0, 0), q->n);
        if (k > 0) tiles += (cs[k] - cs[k - 1] + 63) / 64;
        ts[k] = (int32_t)tiles;
    }
    cs[0] = 0;
    if (c->sm_start_cap < K + 1) {
        c->sm_start_cap = 0;
        HIPCHK(c, c->d_sm_cstart.alloc(sizeof(int64_t) * (DPMM_MAX_CLUSTERS + 1)));
        HIPCHK(c, c->d_sm_tstart.alloc(sizeof(int32_t) * (DPMM_MAX_CLUSTERS + 1)));
        c->sm_start_cap = DPMM_MAX_CLUSTERS + 1;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_sm_cstart, cs.data(), sizeof(int64_t) * cs.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_sm_tstart, ts.data(), sizeof(int32_t) * ts.size(), hipMemcpyHostToDevice, c->stream));
    SampleArgs a{};
    a.i0 = q->i0; a.n = q->n; a.cstart = c->d_sm_cstart; a.tstart = c->d_sm_tstart; a.K = K; a.D = D; a.seed = q->seed;
    a.m = c->d_sm_m; a.At = c->d_sm_At; a.df = c->d_sm_df; a.thr = c->d_sm_thr; a.alias = c->d_sm_alias; a.trials = q->trials;
    a.x = q->x; a.ld = q->ld; a.labels = q->labels;
    if (!mult) {
        HIPCHK(c, launch_sample_niw(a, (int)tiles, c->cus, c->stream));
    } else if (!sparse) {
        HIPCHK(c, launch_sample_mult_dense(a, c->stream));
    } else if (!fill) {
        if (!c->d_sm_cnt) {
            HIPCHK(c, c->d_sm_cnt.alloc(sizeof(int32_t) * (size_t)c->n));
            HIPCHK(c, c->d_sm_bt.alloc(sizeof(int64_t) * ((size_t)csc_scan_tiles(c->n) + 1)));
        }
        a.cnt = c->d_sm_cnt;
        a.labels = nullptr;
        HIPCHK(c, launch_sample_mult_sparse(a, false, c->stream));
        HIPCHK(c, launch_csc_scan(c->d_sm_cnt, q->n, c->d_sm_bt, q->colptr, c->stream));
        HIPCHK(c, launch_sample_add_i64(q->colptr, q->n + 1, q->nnz0, c->stream));
        int64_t kept = 0;
        HIPCHK(c, hipMemcpyAsync(&kept, c->d_sm_bt + csc_scan_tiles(q->n), sizeof(kept), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, sync_stream(c, c->stream));
        *q->nnz_out = kept;
        return DPMM_OK;
    } else {
        a.colptr = q->colptr; a.rowval = q->rowval; a.nzval = q->nzval; a.extent = q->nnz_extent;
        a.labels = nullptr;
        HIPCHK(c, launch_sample_mult_sparse(a, true, c->stream));
    }
    HIPCHK(c, sync_stream(c, c->stream));
    return DPMM_OK;
}

}  // extern "C"
#pragma GCC visibility pop
