// kernels.hpp — launch wrappers of the gfx950 kernels (internal to libpr_amd.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct pr_ctx;

namespace pr {

// ------------------------------------------------------------------ packed layouts
constexpr int SC_NF = 31;                       // rfft bins of the 60 sectors
constexpr int SC_NSLOT = 16;                    // frequency pairs per DB group: (0,30),(1,2),...,(27,28),(29,-)
constexpr int SC_QIMG = SC_NF * 320;            // floats per (channel, 8-query group): [pos(31)][s(5)][lane(64)]
constexpr int SC_DSTEP = 640;                   // floats per (channel, 16-entry DB group, frequency position)
constexpr int SC_DIMG = 2 * SC_NSLOT * SC_DSTEP;  // floats per (channel, 16-entry DB group): 32 positions, the last one zero
// frequency -> position in the packed images (processing order 0,30,1,2,...,29)
__host__ __device__ inline int sc_fpos(int f) { return f == 0 ? 0 : (f == 30 ? 1 : f + 1); }
// split-f16 images (sc_match_h.hip), sizes in BYTES
constexpr int SCH_QROW = 80;                    // one query row: Q hi | Q lo, five 16-byte lane pieces
constexpr int SCH_QBLK = 16 * SCH_QROW;         // (8-query group, frequency): 16 rows, stored in the order of sch_qrow_byte
constexpr int SCH_QIMG = SC_NF * SCH_QBLK;      // 39 680 per (channel, 8-query group)
// Every lane piece of the query image is 16-byte aligned, so sc_match_e reads a tile with ONE ds_read_b128 at an immediate offset from a
// base register per operand pair (the previous image - rows 8..15 shifted by 8 B for ds_read2_b64 - cost a v_add_u32 per read).
// Row r = (Im << 3) | query sits at place sch_qrow_pos(r) of its block.  ds_read_b128 serves the lanes in four groups of 16 - rows 0-3 and
// 12-15 of one lane group k with rows 4-11 of the next - and banks by 16-byte slot mod 16; a row at place p starts at slot 5 p.  The places
// give rows 0-3, 12-15 the slots 0..7 and rows 4-11 the slots 8..15: with the pair offsets below ({0,1,2,0} and {3,4,2,1} slots) that
// leaves 10 two-way collisions in the 8 group accesses of a frequency's two reads - the least any placement of the rows can reach with
// these pair offsets (a group is conflict-free only if the slot sets A of rows 0-3, 12-15 and C of rows 4-11 satisfy A = complement of (C+1) =
// complement of (C+2) in Z16, which no 8-element C does).
__host__ __device__ constexpr int sch_qrow_pos(int row) { return (int)((0xedbafc9865327410ull >> (4 * row)) & 15); }
__host__ __device__ constexpr int sch_qrow_byte(int row) { return SCH_QROW * sch_qrow_pos(row); }     // first byte of a row in its block
static_assert(SCH_QROW % 16 == 0 && SCH_QBLK % 16 == 0 && SCH_QIMG % 16 == 0, "ds_read_b128 needs 16-byte aligned query tiles");
constexpr int SCH_DTILE = 768;                  // one 16x16x32 column operand: 48 lanes x 16 B
constexpr int SCH_DFREQ = 4 * SCH_DTILE;        // Re hi, Re lo, Im hi, Im lo
constexpr int SCH_DIMG = SC_NF * SCH_DFREQ;     // 95 232 per (channel, 16-entry DB group)
// The three split products q_hi d_hi + q_hi d_lo + q_lo d_hi of a frequency's 20 rings are 60 terms; two 16x16x32 MFMAs have 64 K-slots, so
// the matchers run them as TWO operand pairs (not three zero-padded ones) whose 16-byte lane pieces are all contiguous in these images:
//   query row (80 B)   Q hi ring 0..19 | Q lo ring 16..19, 0..15      (the lo half rotated by four rings: Q hi 16..19 and Q lo 16..19 adjoin)
//   DB hi tile         lanes 0-15 D hi 0..7 | 16-31 D hi 8..15 | 32-47 D hi 16..19, zero
//   DB lo tile         lanes 0-15 D lo 0..7 | 16-31 D lo 8..15 | 32-47 D lo 16..19, D hi 16..19   (a copy of the hi values where zeros stood)
//   pair 1:  A lanes (k = lane >> 4) at row + {0, 16, 32, 0}    x  B = hi tile lanes 0-47, lo tile lanes 0-15
//            = Qhi Dhi (rings 0..19) + Qhi Dlo (0..7)                                        [k = 2: Q lo 16..19 meets the tile's zeros]
//   pair 2:  A lanes at row + {48, 64, 32, 16}                 x  B = hi tile lanes 0-31, lo tile lanes 32-47, lo tile lanes 16-31
//            = Qlo Dhi (0..15) + Qhi Dlo (16..19) + Qlo Dhi (16..19) + Qhi Dlo (8..15)
// The single-product kernels read the hi tiles' 48 lanes and the first 40 bytes of a query row - unchanged by this.
__host__ __device__ constexpr int sch_qlo_byte(int ring) { return 40 + ((ring + 4) % 20) * 2; }      // Q lo of a ring, from the row's first byte
__host__ __device__ constexpr int sch_a1_byte(int k) { return k == 3 ? 0 : 16 * k; }                   // pair 1 / pair 2: this lane group's 16 B of the row
__host__ __device__ constexpr int sch_a2_byte(int k) { return k == 0 ? 48 : k == 1 ? 64 : k == 2 ? 32 : 16; }
__host__ __device__ constexpr int sch_b1_byte(int lane) { return lane < 48 ? lane * 16 : SCH_DTILE + (lane - 48) * 16; }   // from the hi tile's first byte
__host__ __device__ constexpr int sch_b2_byte(int lane) { return lane < 32 ? lane * 16 : lane < 48 ? SCH_DTILE + lane * 16 : SCH_DTILE + (lane - 32) * 16; }
// single-product f16 images (PR_SC_ARITH_F16, sc_match_e.hip): the hi halves only
constexpr int SCF_QBLK = 640;                   // (8-query group, frequency): 16 rows x 40 B in row order, NO shift of rows 8..15: the rows are read with ds_read2_b64
                                                // (banks = dword mod 32, 16 consecutive lanes per access) and 10 r mod 32 is distinct for r = 0..15 - an 8-byte shift
                                                // of rows 8..15 made rows 8, 9, 10 collide with rows 5, 6, 7 here (round 6: SQ_LDS_BANK_CONFLICT)
constexpr int SCF_QIMG = SC_NF * SCF_QBLK;      // 20 088 per (channel, 8-query group); a workgroup holds 8 groups = 64 queries
constexpr int SCF_DFREQ = 2 * SCH_DTILE;        // Re, Im
constexpr int SCF_DIMG = SC_NF * SCF_DFREQ;     // 47 616 per (channel, 16-entry DB group) = 2976 B per entry and channel
constexpr int M2_TILE = 96 * 64;                // floats per (channel, 32-row tile): [kq(24)][lane(64)][4]

inline int sc_qgroups8(int m) { return ((m + 31) / 32) * 4; }
inline int sc_qgroups8_f16(int m) { return ((m + 63) / 64) * 8; }
inline int sc_dgroups(int n) { return (n + 15) / 16; }
inline int m2_tiles(int sigs) { return (sigs + 7) / 8; }      // 8 signatures x 4 variants = 32 rows
inline int m2_qtiles(int sigs) { return ((m2_tiles(sigs) + 11) / 12) * 12; }   // query tiles: workgroups take 3 or 4 of them

// Binary intensity channel (SC.cpp:67-72 writes 0 / 1 there): when every row of channel 1 has all of its non-zero entries equal (and
// positive), the row normalised as processSC.m:15-20 does is 1/sqrt(ones) on `ones` bins and every one of the 120 variant products of
// processSC.m:30 is count / sqrt(ones_q ones_d) with an INTEGER count.  The split-f16 pack then also leaves
//   binfo[row] = {sqrt(ones), 1/sqrt(ones)} (floats; {1, 1} for a zero-norm row)
//   bstat[0] |= 1 when a row of channel 1 is not of that form, bstat[1] = max ones, bstat[2..5] = max over the rows of the
//   w-weighted square sum of the f16 rounding residuals of the row's hi spectra (float bits; one slot per frequency block of the pack kernel:
//   their sum bounds the largest row's residual norm^2)
// (bstat is zeroed by the caller in front of every pack) and the matcher runs channel 1 with ONE f16 product per term on the hi halves
// of the same images and rounds count = max x sqrt(ones_q ones_d) to the nearest integer - exact for every pair that passes the test of
// ep_store_round (sc_match_e.hip) under the error bound sc_bin_bound() evaluates from these numbers; the split-f16 kernel otherwise.
constexpr int SC_BSTAT_INTS = 8;
struct ScBin {                    // what the matcher needs of the two sets (device pointers), by value in the kernel arguments
  const int* qstat; const int* dstat;
  const float* qinfo; const float* dinfo;     // [rows][2]
  int* viol;                      // [1] set to `gen` by the single-product pass when a pair fails its rounding test (ep_store_round)
  int gen;                        // the call's sequence number (> 0): the split-f16 pass behind looks for exactly this value, so nobody has to clear the word
  float bconst;                   // (u + gamma)(1 + u) + slack: S and stage-2 constant rounding (pr_api.cpp: create_common)
  float pair_scale;               // 1; tests: PR_SC_BINARY_PAIR_SCALE inflates the bound of the per-pair test only, so that the pass runs and fails it
  int gate;                       // 0: always run; 1: the single-product pass (runs when the bound predicts success); 2: the split-f16 pass behind it (runs when that one did not, or raised viol)
  int chsel;                      // -1: both channels (channel = XCD & 1); 0 / 1: this channel on all XCDs
};
#ifdef __HIPCC__
// The error bound of the single-product pass over a binary channel, evaluated by every workgroup from the same numbers (derivation in
// DESIGN.md §4.0b): with eq, ed the largest w-weighted residual norms of the hi spectra of the two sets, every variant product of a pair is
// within sqrt(ones_q ones_d) x bound of its integer count, bound = eq + ed + eq ed + bconst (1 + eq)(1 + ed).  Returns whether the pass is
// worth running: both sets binary and the largest pair's bound below 0.72 of a count (the pass's actual error, ~6 x 7.6e-5 per unit of
// sqrt(ones_q ones_d) at most, then leaves the per-pair test of ep_store_round room).
__device__ __forceinline__ bool sc_bin_bound(const ScBin& b, float& bound) {
  const int q0 = b.qstat[0], q1 = b.qstat[1], d0 = b.dstat[0], d1 = b.dstat[1];
  const float eq = __builtin_sqrtf(((__int_as_float(b.qstat[2]) + __int_as_float(b.qstat[3])) + __int_as_float(b.qstat[4])) + __int_as_float(b.qstat[5]));
  const float ed = __builtin_sqrtf(((__int_as_float(b.dstat[2]) + __int_as_float(b.dstat[3])) + __int_as_float(b.dstat[4])) + __int_as_float(b.dstat[5]));
  bound = (eq + ed + eq * ed + b.bconst * (1.f + eq) * (1.f + ed)) * 1.001f;
  return q0 == 0 && d0 == 0 && bound * __builtin_sqrtf((float)q1 * (float)d1) < 0.72f;
}
#endif
// sc_pack.hip — processSC.m:15-20 (row L2 normalisation) + per-ring rfft over the 60 sectors, written in the
// MFMA operand layout of `role`.  sig: device [rows][2400] of T.  flags[0] |= 1 if a row has zero norm.
// bad[row] |= 1 << channel for such rows (they are packed as zeros; launch_nan_fixup writes their NaN distances).
void launch_sc_pack(hipStream_t st, const void* sig, int dtype, int rows, int role, float* packed, int groups,
                    const double* twiddle, int* flags, int* bad);
// sc_match.hip — processSC.m:22-33 for both channels.  Writes d_p, d_i device [m][n].
void launch_sc_match(hipStream_t st, const float* qpk, int m, const float* dpk, int n, const float* cst,
                     float* d_p, float* d_i, int nsplit_override);
size_t sc_match_lds_bytes();
void launch_zero_ints(hipStream_t st, int* p, int n);
void launch_fill_ints(hipStream_t st, int* p, int n, int v);
// sc_match_h.hip — the same on the f16 matrix cores with split (hi + lo) operands; packed images from launch_sc_pack_h
void launch_sc_pack_h(hipStream_t st, const void* sig, int dtype, int rows, int role, void* packed, int groups,
                      const double* twiddle, int* flags, int* bad, int single = 0,   // single: hi halves only (SCF_* layout)
                      float* binfo = nullptr, int* bstat = nullptr);                 // binary-channel statistics (ScBin above)
void launch_sc_pack_h_rows(hipStream_t st, const void* sig, int dtype, int rows, int row0, void* packed, int groups, const double* twiddle,
                           int* flags, int* bad, int single, float* binfo, int* bstat);   // rows [row0, row0 + rows) of a DB image (pr_sigset_append)
void launch_sc_match_h(hipStream_t st, const void* qpk, int m, const void* dpk, int n, const void* cst, float* d_p,
                       float* d_i, int nsplit_override, const struct ScBin* bin = nullptr);   // bin: channel selection / gate of a binary-channel call
size_t sc_match_h_lds_bytes();
// sc_match_e.hip — the pair-walk form (no row-exchanged query operand; see the file): single = 0: split-f16 (three products, 4 waves),
// single = 1: one f16 product per term (PR_SC_ARITH_F16), 8 waves = two per SIMD; same packed images and constants as sc_match_h.hip
void launch_sc_match_e(hipStream_t st, const void* qpk, int m, const void* dpk, int n, const void* cst, float* d_p, float* d_i,
                       int nsplit_override, int single, int dgs = 0 /* channel stride of the DB image in 16-entry groups when it is not sc_dgroups(n): an appendable set */,
                       int sweep = 1 /* split-f16, m > 8: 1 = query groups resident in LDS, DB tiles streamed; 2 = one DB group resident, query tiles streamed; 0 = by shape */);
int sc_dbr_ranges(int m, int DG, int chans, int cus);     // query ranges of the DB-resident sweep (the tail rule, sc_match_e.hip)
bool sc_dbr_auto(int m, int n);                          // the shapes at which `auto` takes the DB-resident sweep
// split-f16 images whose channel 1 may be binary (ScBin above): channel 0 in split-f16; channel 1 by the single-product kernel on the hi
// halves with integer rounding when the sets' statistics allow it, in split-f16 otherwise - the decision is taken ON THE DEVICE by every
// workgroup from the same numbers (no host round trip: the two channel-1 launches are both issued, one of them leaves at once).
// ev (or null): four events recorded around the launches (channel 0 | channel 1 single product | channel 1 split)
// (Measured and dropped: the channel-0 launch of an online call and the binary pass on two streams at once - 0.302 -> 0.308 ms at m = 1,
// 0.310 -> 0.337 at m = 8: sc_match_h's workgroups fill the LDS of their CUs, the two kernels do not run side by side, and the event hand-offs cost.)
void launch_sc_match_e_bin(hipStream_t st, const void* qpk, int m, const void* dpk, int n, const void* cst, float* d_p, float* d_i,
                           int nsplit_override, ScBin bin, hipEvent_t* ev, int online_h = 0 /* m <= 8: sc_match_h.hip's one-group form (PR_SC_ONLINE=h, read once at pr_create) */, int dgs = 0 /* as in launch_sc_match_e */, int sweep = 1 /* as in launch_sc_match_e */);

// m2dp_match.hip — processM2DP.m:12-22 for both channels.
void launch_m2dp_pack(hipStream_t st, const void* sig, int dtype, int sigs, float* packed, int tiles);
void launch_m2dp_match(hipStream_t st, const float* qpk, int m, const float* dpk, int n, float* d_p, float* d_i);
// m2dp_match_h.hip — the same with split-f16 operands on the f16 matrix cores (tiles of the same size, packed by launch_m2dp_pack_h)
void launch_m2dp_pack_h(hipStream_t st, const void* sig, int dtype, int sigs, void* packed, int tiles, int sg0 = 0 /* first signature's place in the image */);
void launch_m2dp_match_h(hipStream_t st, const void* qpk, int m, const void* dpk, int n, float* d_p, float* d_i, int single = 0 /* hi halves only */,
                         int dts = 0 /* channel stride of the DB image in tiles when it is not m2_tiles(n): an appendable set */);

// fuse_select.hip — run_test.m:38-41,47-53,57
// scratch (select_scratch_bytes(), or null): lets a call with few query rows cut every row into slices (grid m x P) instead of one workgroup per row
size_t select_scratch_bytes();
void launch_row_moments(hipStream_t st, const float* d_p, const float* d_i, int m, int n, double* mom, void* scratch = nullptr);
void launch_fuse_select(hipStream_t st, const float* d_p, const float* d_i, int m, int n, const double* mom_all,
                        int G, int q_row0, int db_row0, int mask_width, double p_weight, int k, int32_t* idx,
                        float* score, const float* e_p = nullptr, const float* e_i = nullptr, const double* mom2_all = nullptr, void* scratch = nullptr,
                        double* score64 = nullptr /* the same scores widened to f64 [m][k] */);
// launch_row_moments + launch_fuse_select of one shard (G = 1, one channel pair) - in ONE sweep of the rows (moments_select_kernel) where
// the selection is the whole-row one with up to 16 results; mom, idx, score, score64 come out bit for bit as from the two calls.
// fell (device, or null): += the rows the fused kernel answered through a second sweep
void launch_moments_select(hipStream_t st, const float* d_p, const float* d_i, int m, int n, double* mom, int q_row0, int db_row0, int mask_width,
                           double p_weight, int k, int32_t* idx, float* score, double* score64, void* scratch, unsigned long long* fell);

// rerank.hip — NaN rows / columns of zero-norm signatures (processSC.m:16,19), the fp64 re-evaluation of the fp32
// selection's survivors (processSC.m:15-33 / processM2DP.m:12-22 + run_test.m:40 per pair) and the k-way shard merge
void launch_nan_fixup(hipStream_t st, float* d_p, float* d_i, int m, int n, const int* qbad, const int* dbad);
// p5 [m][5][kin] (p5_all [G][m][5][kin]): per query the candidates' scores [kin] and their four exact channel distances [4][kin] (SC structure,
// SC intensity, M2DP count, M2DP intensity; NaN in the first = not evaluated) - what a shard knows after its re-evaluation (rerank.hip)
void launch_rerank(hipStream_t st, const void* q_sc, const void* db_sc, int sc_dt, const void* q_m2, const void* db_m2, int m2_dt,
                   const double* mom_sc, const double* mom_m2, int m, int n_local, int G, int q_row0, int db_row0, int mask_width,
                   double p_weight, int kin, const int32_t* idx_in, double* p5, unsigned* tick /* [cap] zeros (left zero) | [cap] work list | [1] */, size_t tick_cap /* >= m kin */, int k, int32_t* idx, double* score,
                   float* score32, const double* cand_sc32, double eps_d = 0.0, double order_floor = 0.0,
                   double order_noise = 0.0, int32_t* order_flags = nullptr);   // order_flags [m]: the order check of launch_order_check on the result; cand_sc32: the candidates' all-pairs-pass scores (ascending) or null: prunes hopeless candidates; eps_d: that pass's distance error bound (0: the fp32-grade 1e-6 with a 64x margin)
// the sharded form: scores + distances of the candidates THIS shard owns (NaN elsewhere), then owner-wise combination + selection
void launch_rerank_partial(hipStream_t st, const void* q_sc, const void* db_sc, int sc_dt, const void* q_m2, const void* db_m2, int m2_dt,
                           const double* mom_sc, const double* mom_m2, int m, int n_local, int G, int q_row0, int db_row0, int mask_width,
                           double p_weight, int kin, const int32_t* idx_in, double* p5, unsigned* tick, size_t tick_cap, const double* cand_sc32, int k,
                           double eps_d = 0.0);
// PR_SC_ARITH_F16: flags[q] = 1 where the candidate list does not provably contain the exact top-k (rerank.hip), count += number of flags
void launch_margin_check(hipStream_t st, const double* mom_sc, const double* mom_m2, int G, int m, double p_weight, int kin,
                         const double* cand_sc, int k, const double* score, double eps_d, int32_t* flags, int32_t* count,
                         const int32_t* order_flags, double eps_floor, double noise /* the order check's constants of this arithmetic: sigma slack of the containment test */);
// flags[q] = 1 where the order of the re-evaluated candidates (the selected k and the best one left out) could change under the sigma error
// of the all-pairs pass (per channel eps_floor + noise / sigma: noise = the largest error of one distance; statistics from mom_* [Gmom][m][2][3])
// + bit 1 where the candidate list (cand_sc [m][kin]: its all-pairs-pass scores, ascending; score_sel [m][k]: the exact scores of the k selected;
// both or neither) does not provably hold the exact top-k of the whole row
void launch_order_check(hipStream_t st, const double* mom_sc, const double* mom_m2, int Gmom, const int32_t* cand_idx, const double* p5_all,
                        int G, int m, int kin, int k, const int32_t* idx_sel, double p_weight, double eps_floor, double noise, int32_t* flags,
                        const double* cand_sc = nullptr, const double* score_sel = nullptr);
// The flagged queries (order not certain under the pass's sigmas | candidate list not provably complete: rerank.hip) answered from their EXACT
// rows, stream-ordered (exact_row.hip): flags -> ascending list + count; per pass of RESOLVE_SLOTS list slots from `offset`
//   launch_xrow         this shard's fp64 distances of the slot's query to every entry (rows [RESOLVE_SLOTS][4][n_local]) and their exact
//                       (count, mean, M2) per channel (exact [m][4][3]; partial: scratch [RESOLVE_SLOTS][RESOLVE_NB][4][3])
//   launch_xrow_select  the k smallest (fused fp64 score, global index) of the slot's row under the statistics of all shards (exact_all
//                       [G][m][4][3]) and the mask -> sel [RESOLVE_SLOTS][2][k] (scores | indices as doubles); with sel = null (one shard)
//                       straight into idx / score [m][k], out_mom_* rows [m][2][3] patched with the exact moments
//   launch_xrow_merge   sel_all [G][RESOLVE_SLOTS][2][k] of all shards -> idx / score of the slots' queries
constexpr int RESOLVE_SLOTS = 64;
constexpr int RESOLVE_NB = 2048;
constexpr int RESOLVE_SMALL_M = 1024;            // calls of up to this many queries: the kernels scan the flags themselves (no compaction launch)
int exact_partial_blocks(int n_local);
void launch_flag_compact(hipStream_t st, const int32_t* flags, int m, int32_t* list, int32_t* cnt);
// compacted: list / cnt are already there (launch_flag_compact: the host-synchronising form runs several passes over one list)
void launch_xrow(hipStream_t st, const void* q_sc, const void* db_sc, int sc_dt, const void* q_m2, const void* db_m2, int m2_dt,
                 const double* mom_sc, const double* mom_m2, int G, int m, int n_local, const int32_t* flags, int32_t* list, int32_t* cnt,
                 int offset, bool compacted, double* partial, double* exact, double* rows, unsigned* tick, int* dflags,
                 int last_pass /* no pass follows: flagged queries beyond this pass's 64 are reported in dflags[3] */, double* qspec /* [xrow_qspec_doubles()] scratch: the slots' query spectra */, const double* tw /* cos | sin of 2 pi t / 60 */,
                 int direct /* 1: the reference's own formulation instead of the spectral form */);
size_t xrow_qspec_doubles();
hipError_t xrow_set_twiddles(const double* cos60, const double* sin60);   // once per device, before the first launch_xrow (constant memory of exact_row.hip)
void launch_xrow_select(hipStream_t st, const int32_t* flags, const int32_t* list, const int32_t* cnt, int offset, const double* exact_all, int G,
                        int m, int n_local, int q_row0, int db_row0, int mask_width, double p_weight, int has_sc, int has_m2, int k,
                        const double* rows, double* part /* [xrow_select_part_doubles(m, k)] scratch: the row slices' lists */, double* sel, int32_t* idx,
                        double* score, double* out_mom_sc, double* out_mom_m2);
size_t xrow_select_part_doubles(int m, int k);
void launch_xrow_merge(hipStream_t st, const int32_t* flags, const int32_t* list, const int32_t* cnt, int offset, const double* sel_all, int G, int m,
                       int k, int32_t* idx, double* score);
void launch_rerank_finish(hipStream_t st, const int32_t* cand_idx, const double* p5_all, int G, int m, int kin, int k, int32_t* idx,
                          double* score);
void launch_widen(hipStream_t st, const float* a, long long n, double* b);
void launch_merge_topk(hipStream_t st, const int32_t* idx_all, const double* score_all, int G, int m, int k, int32_t* idx, double* score);

// align.hip — the argmin variant of a (query, DB entry) pair per channel (processSC.m:22-33, processM2DP.m:12-22, processDELIGHT.m:7-37)
void launch_align(hipStream_t st, const void* q_sc, const void* db_sc, int sc_dt, const void* q_m2, const void* db_m2, int m2_dt, int m,
                  int n_local, int db_row0, int k, const int32_t* idx, int32_t* variant /* [m][k][4] */, double* dist /* [m][k][4] */);
void launch_delight_align(hipStream_t st, const void* q, const void* db, int dt, int m, int n_local, int db_row0, int k, const int32_t* idx,
                          int32_t* variant /* [m][k] */, double* dist /* [m][k] */);

// sc_gen.hip / m2dp_gen.hip — pts_align.h:7-46 + SC.cpp:12-76 / M2DP.cpp:38-109 (+ test_m2dp.cpp:44-68)
void launch_ave_chain(hipStream_t st, const float* inten, const int64_t* offs, int N, float* ave /* [N] or NULL */,
                      double* frames = nullptr /* non-NULL: also frames[c][14] = the average, [15] = 1 (frames.hpp) */);
void launch_cloud_frames(hipStream_t st, const double* xyz, const int64_t* offs, int N, double* frames);
// the one-HBM-pass path of SC generation (see sc_gen.hip): a batch of clouds small enough for the Infinity Cache, W workgroups per cloud
constexpr int SC_MAX_W = 16;                     // slices per cloud
constexpr int SC_MAX_SPLIT_CLOUDS = 1024;        // clouds per batch when W > 1
constexpr size_t SC_SCRATCH_PER_STREAM = (size_t)2 * SC_MAX_SPLIT_CLOUDS * 4 + (size_t)SC_MAX_SPLIT_CLOUDS * SC_MAX_W * 9 * 8 +
                                         (size_t)768 * (1200 * 4 + 3 * 1200 * 8);   // tickets + partial moments + partial grids (nb * W <= 768)
size_t sc_generate_scratch_bytes();
void launch_sc_batch(hipStream_t st, const double* xyz, const float* inten, const int64_t* offs, int c0, int c1, int W, double max_rho,
                     double* frames, char* scratch, double* out);
size_t sc_cluster_scratch_bytes(int ncl, int CW);
int sc_cluster_points_per_workgroup();
int* launch_sc_cluster(hipStream_t st, const double* xyz, const float* inten, const int64_t* offs, int N, double max_rho, int CW, int ncu,
                       char* scratch, double* frames, double* out);
void launch_sc_finish(hipStream_t st, const float* ave, int N, double* out);
void launch_sc_bin(hipStream_t st, const double* xyz, const float* inten, const int64_t* offs, int N, double max_rho,
                   const double* frames, const float* ave /* NULL: out[c][1200..] = bin means, launch_sc_finish applies the averages */, double* out,
                   int ave_in_frames = 0 /* with ave = NULL: the averages are frames[c][14] */);
void launch_m2dp_bin_svd(hipStream_t st, const double* xyz, const float* inten, const int64_t* offs, int N,
                         double max_rho, const double* frames, const float* ave, const double* planes, double* mats,
                         double* out, int* flags /* [1] |= 1: a leading singular pair is not unique */,
                         int* svd_rows /* [0] += 1 and [1 + slot] = signature row (cloud * 4 + variant) for each such pair */,
                         hipStream_t st2 = nullptr, hipEvent_t* ev_bin = nullptr, hipEvent_t* ev_svd = nullptr /* [2] each: more than one
                         batch of clouds -> the singular pairs of a batch run on st2 beside the binning of the next (see m2dp_gen.hip) */);
constexpr int M2DP_SVD_ROWS_CAP = 1024;
constexpr double M2DP_SVD_TIE_TRACE = 1.001;   // trace(G^256) above this: the leading pair is (nearly) tied (m2dp_svd_kernel; sigma_1 / sigma_2 < ~1.0136)
size_t m2dp_generate_scratch_bytes(int N);

// plain_match.hip — processGIST.m:1-10, processBoW.m:1-38 (h1, h2: device, row-major doubles; BoW rows alternate ids | weights)
void launch_gist_distance(hipStream_t st, const double* h1, int m, const double* h2, int n, int cols, float* dist);
void launch_bow_distance(hipStream_t st, const double* h1, int m, const double* h2, int n, int cols, float* dist);
// delight.hip — DELIGHT.cpp:8-24, processDELIGHT.m:1-38
void launch_delight_gen(hipStream_t st, const double* xyz, const float* inten, const int64_t* offs, int N,
                        const double* frames, double* out);
void launch_delight_pack(hipStream_t st, const void* sig, int dtype, int sigs, float* packed, unsigned* mask);
void launch_delight_match(hipStream_t st, const float* q, int m, const float* db, const unsigned* dbmask, int n, float* dist);
// gist_gen.hip — libgist.cpp:914-951 (bw_gist_scaletab) for 256 x 256 images: n images (u8 or f32, [n][256][256]) -> out [n][nf nb^2].
// circ: [GIST_LD][GIST_LD] whitening circulant (266 x 266 valid), gabor: [nf][256][256], tw: W256^m (m < 256, forward sign);
// scratch: gist_scratch_floats(chunk >= n, nf, nb) floats.  Stream-ordered, allocates nothing.
constexpr int GIST_LD = 272;      // row stride of the padded 266 x 266 planes
constexpr int GIST_PAIRS = 128;   // (image, filter) pairs per Gabor launch: their 256 x 256 c64 intermediates (64 MiB) stay cache-resident
size_t gist_scratch_floats(int chunk, int nf, int nb);
void launch_gist(hipStream_t st, const void* img, bool u8, int n, int nb, int nf, const float* circ, const float* gabor,
                 const float2* tw, float* scratch, float* out);
void gist_release(void* state);                 // gist.cpp: frees a context's GIST tables and scratch (pr_destroy, streams idle)
// bow_gen.hip — TemplatedVocabulary::transform (TemplatedVocabulary.h:1127-1260) over a vocabulary tree in BFS order: node b's children
// are child[b].x .. child[b].x + child[b].y - 1 (contiguous, file order), desc [nodes][32 B], word / weight of each node.
//   launch_bow_descend: feature f of n_desc -> node[f] (the childless node its descent ends on), lanes per feature 1..16 (a power of 2);
//                       feat_words (or null) [f] = word[node[f]]
//   launch_bow_aggregate: per image (offs clamped into [0, n_desc]) the BowVector of the reference's order, written as ids / values rows
//                       of out [2N][cols]; n_words (or null) [i] = distinct words; flags[0] = 1 when one has more than cols.
//   scratch: wgt [n_desc] f64 (set by aggregate's fill), vals [n_desc] f64, gkeys [2 n_desc] u64 (images of more than BOW_LDS_KEYS descriptors).
constexpr int BOW_LDS_KEYS = 8192;
void launch_bow_descend(hipStream_t st, const uint8_t* desc, int64_t n_desc, const uint4* vdesc, const int2* child, const int* word,
                        int lanes, int* node, int* feat_words);
void launch_bow_aggregate(hipStream_t st, const int64_t* offs, int N, int64_t n_desc, const int* node, const int* word, const double* weight,
                          int weighting, int scoring, int cols, double* wgt, double* vals, unsigned long long* gkeys, double* out,
                          int* n_words, int* flags);   // node null: a vocabulary without words, every row empty
void launch_bow_fill_words(hipStream_t st, int* feat_words, int64_t n, int v);
void bow_release(void* state);                  // bow.cpp: frees a context's device vocabularies and scratch (pr_destroy, streams idle)
// bow_match.hip — the inverted-file BoW matcher (see the file header); all pointers are device pointers
void launch_bow_rows_check(hipStream_t st, const double* rows, int n, int cols, int n_words, int row_name0, int* counts,
                           unsigned long long* total, int* bad);      // counts may be null (validation only)
void launch_bow_scatter(hipStream_t st, const double* rows, int n, int cols, int j0, unsigned long long* cursor, int* prow, double* pw);
int bow_scan_tiles(int nw);                     // tile sums the scan needs
void launch_bow_scan(hipStream_t st, const int* counts, int nw, unsigned long long* tsum, unsigned long long* off, unsigned long long* cursor);
void launch_bow_fold(hipStream_t st, int nw, const unsigned long long* moff, const int* mrow, const double* mw, const unsigned long long* toff,
                     const int* trow, const double* tw, unsigned long long* noff, int* nrow, double* nwt);
void launch_bow_score(hipStream_t st, int threads, const double* q, int m, int cols, int n_words, int q_row0, const unsigned long long* moff,
                      const int* mrow, const double* mw, const unsigned long long* toff, const int* trow, const double* tw, int n, int db_row0,
                      int mask_width, int k, double* acc, int32_t* idx, double* score, int* flag);   // k = 0: acc rows [m][n] keep d
// gist_match.hip — the two-stage exact GIST matcher (see the file header); all pointers are device pointers.  KS = K-steps of 16 columns
// (a multiple of 4), S = DB slabs, C = list length per (query, slab), S * C <= 2048.
void launch_gist_mean(hipStream_t st, const double* rows, int nr, int cols, double* mu);
void launch_gist_pack(hipStream_t st, const double* rows, int n, int cols, int KS, const double* mu, int row0, void* img, float* nd, float* rs,
                      unsigned* stat /* null (queries) | [0] max nd, [1] max rs as float bits */);
size_t gist_coarse_lds_bytes(int KS, int C);
void launch_gist_coarse(hipStream_t st, const void* qpk, const float* qn, int m, const void* dpk, const float* dn, int n, int KS, int S, int C,
                        int q_row0, int db_row0, int mask_width, int* cand /* [m][S][C] local rows, -1 = empty */, float* wout /* [m][S] */);
void launch_gist_rerank(hipStream_t st, const double* q, const double* raw, int cols, int KP, int m, int S, int C, const int* cand,
                        const float* wout, const float* qn, const float* qr, const unsigned* dstat, int db_row0, int k, int32_t* idx,
                        double* score, int* flags /* [m] 1: not provably complete */);
void launch_gist_compact(hipStream_t st, const int* flags, int m, int* list, int* cnt /* [0] = count, [1] += count */);
void launch_gist_fill(hipStream_t st, int* p, int n, int v);
void launch_gist_xdist(hipStream_t st, const double* q, const double* raw, int cols, int n, const int* list, const int* cnt, int offset,
                       int direct_count, int cap, double* out, size_t ld, int q_row0, int db_row0, int mask_width);
void launch_gist_xselect(hipStream_t st, const double* rows, size_t ld, int n, const int* list, const int* cnt, int offset, int cap, int db_row0,
                         int k, int32_t* idx, double* score);
// delight_match.hip — the two-stage exact DELIGHT matcher (see the file header); all pointers are device pointers.  S = DB slabs,
// C = list length per (query, slab) <= 136, S * C <= 2048.  Selection and compaction of the exact rows: launch_gist_xselect / _compact.
void launch_delight_dpack(hipStream_t st, const double* rows, int n, int row0, float* img, unsigned* mask, int* okflag,
                          unsigned* stat /* null (queries) | [0] += rows that are not coarse-exact */);
void launch_delight_coarse(hipStream_t st, const float* q, int m, const float* db, const unsigned* dbmask, int n, int S, int C, int q_row0,
                           int db_row0, int mask_width, int* cand /* [m][S][C] local rows, -1 = empty */, float* ckey /* [m][S][C] */,
                           float* wout /* [m][S] */);
void launch_delight_rerank(hipStream_t st, const double* q, const double* raw, int m, int S, int C, const int* cand, const float* ckey,
                           const float* wout, const int* qok, const unsigned* dstat, int db_row0, int k, int32_t* idx, double* score,
                           int* flags /* [m] 1: not provably complete */);
void launch_delight_xdist(hipStream_t st, const double* q, const double* raw, int n, const int* list, const int* cnt, int offset,
                          int direct_count, int cap, double* out, size_t ld, int q_row0, int db_row0, int mask_width);
// eval.hip — the evaluation half of run_test.m on the device (see the file header); all pointers are device pointers
constexpr int EVAL_TILE = 256;                  // gt2 rows a workgroup stages in LDS at a time (cols <= 3)
constexpr int EVAL_MAX_COLS = 3 * EVAL_TILE;    // widest position row: the generic kernel's tile holds at least one
constexpr int EVAL_SCAN = 1024;                 // items per workgroup of the two-level integer scans
struct EvalScalars { double auc, top_recall; int32_t n_gt, n_detected; };   // pr_precision_recall_dev's d_scalars
// run_test.m:3-16: per query the first minimum over gt2 rows [s chunk, (s + 1) chunk) for s < nsplit, written at [s][m] of out_d / out_j;
// chunk is a multiple of EVAL_TILE; rq = 1 | 4 queries per lane (4: cols <= 3 only)
void launch_eval_gt(hipStream_t st, const double* gt1, int m, const double* gt2, int n, int cols, int mask_width, int chunk, int nsplit, int rq,
                    double* out_d, int* out_j);
void launch_eval_gt_combine(hipStream_t st, const double* part_d, const int* part_j, int m, int nsplit, double* min_d, int* min_j);
// run_test.m:17-20: the pairs with min_d < thr in ascending i (two-level scan: loc [m], bsum [2 blocks + 2] scratch); lp may be null
void launch_eval_gt_pairs(hipStream_t st, const double* min_d, const int* min_j, int m, double thr, int* loc, int* bsum, int32_t* lp, int32_t* n_gt);
// run_test.m:58-85.  cnt / rank / bidx / cls / loc [m], bsum [2 blocks + 2], prec / rec / term [m] scratch (prec, rec may be the caller's)
void launch_eval_sweep(hipStream_t st, const double* diff_v, const int32_t* diff_idx, int ld, int m, const double* gt1, const double* gt2, int n,
                       int cols, double thr, int* cnt, int* rank, int* bidx, int* cls, int* loc, int* bsum, double* prec, double* rec,
                       double* term, EvalScalars* scal, int32_t* lp_detected);
// sum over i < m - 1 of ((r[i+1] - r[i]) * (p[i] + p[i+1])) / 2, added in that order from 0 by one lane; term [m] scratch
void launch_eval_trapz(hipStream_t st, const double* rec, const double* prec, int m, double* term, double* out);
void eval_release(void* state);                 // eval_dev.cpp: frees a context's evaluation scratch (pr_destroy, streams idle)
// icp.hip — point-to-point ICP of matched cloud pairs (see the file header); all pointers are device pointers
constexpr int ICP_TILE = 256;                   // target rows a workgroup stages in LDS at a time
constexpr int ICP_SUMS = 17;                    // fp64 sums per chunk: n, sum d2, sum p' [3], sum q [3], sum p' q^T [3][3] (p', q about the chunk's pivot)
constexpr int ICP_PARTIAL = ICP_SUMS + 3;       // a chunk's record: its sums and its pivot [3]
enum { ICP_RUNNING = -1, ICP_CONVERGED = 0, ICP_MAX_ITER = 1, ICP_TOO_FEW = 2, ICP_DEGENERATE = 3, ICP_NO_PAIR = 4 };   // PR_ICP_* of the header
struct IcpStats { double fitness, rmse; int32_t n_inl, iters, status, pad; };   // pr_icp_pairs_dev's stats record
struct IcpParams { double tol_rmse, tol_fitness; int min_inliers; };
// two CSR cloud sets and c pairs (pair_src[i] of the query set onto pair_dst[i] of the DB set; -1 or out of range: none); clouds are read
// up to max_src / max_dst points
struct IcpClouds {
  const double* xyz_q; const int64_t* offs_q; int Nq;
  const double* xyz_d; const int64_t* offs_d; int Nd;
  const int32_t* pair_src; const int32_t* pair_dst; int c;
  int max_src, max_dst;
};
// rq = 1 | 4 source points per lane; nsplit target ranges of whole tiles (> 1: slots [nsplit][c][ld] + the combining launch);
// ld = row stride of the per-pair arrays; chunk_pts = source points per partial (256 rq, 256 with a split), nchunks = partials per pair
struct IcpGeometry { int rq, nsplit, ld, chunk_pts, nchunks; };
void launch_icp_offsets(hipStream_t st, const IcpClouds& A, long long* out_offs /* [c + 1] */);
void launch_icp_init(hipStream_t st, const IcpClouds& A, const double* T0, double* T, IcpStats* stats, int* done, double* prev /* [c][2] */);
// one correspondence pass under T [c][3][4]: nn_d / nn_j rows at base[pair] (or pair * ld); done (or null): pairs to skip;
// part (or null) [c][nchunks][ICP_PARTIAL]: the inliers' (d2 < mc2) sums per chunk
void launch_icp_nn(hipStream_t st, const IcpClouds& A, const IcpGeometry& g, const double* T, const int* done, double* slot_d, int* slot_j,
                   const long long* base, double* nn_d, int* nn_j, double mc2, double* part);
void launch_icp_finish(hipStream_t st, const IcpClouds& A, const IcpGeometry& g, const double* part, const IcpParams& P, int final_pass, double* T,
                       IcpStats* stats, int* done, double* prev);
// icp_grid.hip — the exact uniform-grid correspondence search.  Per pair slot: the box of the finite target points, the
// cell edge h and the cells per axis; `ends` [c][cells] ints (counts, then exclusive starts, after the scatter the cells' ends) and
// `sorted` [c][max_dst] ints (the finite target points' indices, cell by cell)
struct IcpGridBox { double x0[3], h; int n[3], flags; };      // flags 1: h is not finite - one cell holds every finite point
struct IcpGrid { IcpGridBox* box; int* ends; int* sorted; int cells, G; };   // cells per pair slot (>= (G + 1)^3), G: the host's cells per axis
constexpr double ICP_GRID_SLACK = 1.0 + 0x1p-10;               // h >= max_corr * ICP_GRID_SLACK
// box -> clear -> count -> scan -> scatter: five launches on st, no read-back
void launch_icp_grid_build(hipStream_t st, const IcpClouds& A, const IcpGrid& gr, double max_corr);
// one pass: 27 cells per source point, results (j, d2) where d2 < mc2, (-1, +Inf) elsewhere, at base[pair] (or pair * ld); part (or
// null) [c][nchunks][ICP_PARTIAL]: the sums of chunks of 256 points (icp_common.hpp's chunk_sums, as the brute-force combining launch)
void launch_icp_grid_probe(hipStream_t st, const IcpClouds& A, const IcpGrid& gr, const double* T, const int* done, int ld, const long long* base,
                           double* nn_d, int* nn_j, double mc2, double* part, int nchunks);
// the brute-force pass's rows masked to d2 < mc2: (-1, +Inf) elsewhere
void launch_icp_radius_mask(hipStream_t st, const IcpClouds& A, const long long* base, double* nn_d, int* nn_j, double mc2);
void icp_release(void* state);                  // icp.cpp: frees a context's ICP scratch (pr_destroy, streams idle)
// icp.cpp: pr_icp_pairs_dev's argument checks (cloud sets, bounds, parameters) for a caller that brings pair lists of its own: PR_OK or
// PR_EINVAL with the context's error text set, nothing touched
int icp_check_pairs_args(pr_ctx* ctx, const char* fn, const void* xyz_q, const void* offs_q, int32_t Nq, const void* xyz_d, const void* offs_d,
                         int32_t Nd, int32_t c, int64_t max_src, int64_t max_dst, int32_t max_iter, double max_corr, double tol_rmse,
                         double tol_fitness, int32_t min_inliers);
// pose.hip — the pose seed of matched pairs and the choice among a pair's refined hypotheses (see the file header)
// slots [m][k][H]: hypothesis h of pair p reads variant[p * stride + h]; angles: cos | sin of k 2 pi / 60, k = 0 .. 60 (pose_seed.hpp)
void launch_pose_seed(hipStream_t st, int type, const double* frames_q, int m, const double* frames_db, int n_local, int db_row0, int k,
                      const int* idx, const int* variant, int stride, int H, const double* angles, double* T0, int* pair_src, int* pair_dst);
void launch_verify_select(hipStream_t st, const double* T_h /* [c][H][3][4] */, const IcpStats* stats_h /* [c][H] */, int c, int H,
                          double min_fitness, double max_rmse, double* T, IcpStats* stats, unsigned char* accepted, int* hyp);
void pose_release(void* state);                 // pose.cpp: frees a context's angle tables and verify scratch (pr_destroy, streams idle)
// pr_api.cpp: what gist.cpp and bow.cpp need of a context
hipStream_t ctx_stream(pr_ctx* ctx);
int ctx_device(pr_ctx* ctx);
void ctx_set_error(pr_ctx* ctx, const char* msg);
void*& ctx_gist(pr_ctx* ctx);
void*& ctx_bow(pr_ctx* ctx);
void*& ctx_eval(pr_ctx* ctx);
void*& ctx_icp(pr_ctx* ctx);
void*& ctx_pose(pr_ctx* ctx);
void* ctx_seq_scratch(pr_ctx* ctx);           // the lists of pr_seq_select_dev's column parts (seqmatch.hpp: seq_scratch_bytes)
int* ctx_bow_flag(pr_ctx* ctx);                 // [1] device word: a BoW row was truncated (PR_WARN_BOW_TRUNCATED at pr_take_warnings)
int* ctx_bow_rows_flag(pr_ctx* ctx);            // [1] device word: a non-conforming BoW query row (PR_WARN_BOW_ROWS at pr_take_warnings)

// prestage.hip — utils/pts_preprocess.h:135-232 on the GPU (see the file header); all pointers are device pointers
int64_t prestage_cells(double range, int polar);          // dense cell-table length per pose
void launch_death(hipStream_t st, const double* xyz, const int* birth, int64_t T, const double* W, const unsigned char* emit,
                  const int* next_reset, double range, int* death);
void launch_members(hipStream_t st, int E, const int* death, const int* pose_of, const int64_t* first_alive, const int64_t* cursor,
                    const int64_t* off, int* cnt, int* list);
void launch_cells(hipStream_t st, const double* xyz, const int* list, const int64_t* off, const int* pose_of, int e0, int e1,
                  int64_t s0, int64_t s1, const double* W, double range, int polar, int64_t C, int* cell, unsigned long long* val,
                  unsigned long long* tval, unsigned* tfirst, unsigned* tbest);
void launch_keys(hipStream_t st, const int64_t* off, int e0, int e1, int64_t C, const int* cell, const int* list, const unsigned* tfirst,
                 const unsigned* tbest, int* keys, int* win, int* nkeys);
void launch_order(hipStream_t st, int E, const int64_t* off, const int* nkeys, const int* keys, const int* sched_cnt, const int* sched_nb,
                  int nsched, int* next, const int64_t* boff, int* bkt, int* order);
void launch_gather(hipStream_t st, int E, int64_t total, const int64_t* off, const int64_t* ooff, const int* pose_of, const int* order,
                   const int* win, const double* xyz, const float* inten, const double* W, double range, double* oxyz, float* oint,
                   double* frames /* non-NULL: one workgroup per cloud, which also leaves the cloud's PCA frame [E][16] (frames.hpp) */);

// The pre-stage's cell grid (prestage_common.hpp: make_grid / cell_of)
struct Grid { double range, step[3]; int dim[3]; int polar, azi_bins; double inv; };

// window.hip — the pre-stage one keyframe at a time.  WinView: what the kernels of a push need of a pr_window (window.cpp);
// every pointer is device memory allocated at create.
constexpr int WIN_STATE_WORDS = 16;
constexpr int WIN_OVERFLOW = 1;              // = PR_WINDOW_OVERFLOW
constexpr int WIN_ORDER_GLOBAL = 2;          // = PR_WINDOW_ORDER_GLOBAL
constexpr int WIN_ORDER_LDS_INTS = 40960;    // the order kernel's LDS scratch (160 KB): next[K] + bkt[bucket count] live there when they fit
struct WinView {
  Grid grid;
  int cap, max_new, max_out, nsched;
  int64_t C;                                 // cells of the dense table
  int* st;                                   // [WIN_STATE_WORDS] state words
  double* xyz[2];                            // [cap][3] world points of the set, ping-pong
  float* inten[2];                           // [cap]
  int *bcnt, *boff, *kcnt, *koff;            // [ceil(cap / 256)] per-workgroup counts and their exclusive scans (survivors | keys)
  int* cell;                                 // [cap] per member
  unsigned long long* val;                   // [cap]
  unsigned long long* tval;                  // [C] per cell: minimum ordering value, first member, winner
  unsigned *tfirst, *tbest;
  int *keys, *win, *next, *order;            // [cap]
  int* bkt;                                  // [largest bucket count of the schedule]
  const int *sched_cnt, *sched_nb;           // [nsched] libstdc++'s growth schedule (probe_bucket_schedule)
};
void window_fill_grid(WinView& v, double range, int polar);
void launch_window_reset(hipStream_t st, const WinView& v);
void launch_window_push(hipStream_t st, const WinView& v, const double* pose, const double* xyz_new, const float* inten_new,
                        const int* n_new_dev, int max_new, double* out_xyz, float* out_inten, int64_t* out_offs, double* out_frame, int* info);

// map.hip — the resident keyframe map.  MapView: the caller's seven buffers, the create capacities and the plan scratch of
// a pr_map (map.cpp).  plan [MAP_PLAN_HEAD + 3 max_append + 1] int64: the head words below, then cum [max_append + 1] (the clouds' first
// points counted from the call's first point), dst [max_append] (first point in the map's xyz; -1: no points stored) and end [max_append]
// (the map's offs behind the cloud's row).
constexpr int MAP_OVERFLOW = 1;              // = PR_MAP_OVERFLOW
constexpr int MAP_DROPPED = 2;               // = PR_MAP_DROPPED
constexpr int MAP_PLAN_HEAD = 6;             // plan[0] rows appended, [1] first row | -1, [2] points the copy covers, [3] flags of this call,
                                             // [4] keyframes before the call, [5] 0: the call was switched off by d_emitted
struct MapView {
  double* xyz; float* inten; int64_t* offs; double* frames; double* poses; int* ids; int* state;
  int kcap, max_cloud, max_append;
  int64_t pcap;
  int64_t* plan;
};
inline size_t map_plan_words(int max_append) { return (size_t)MAP_PLAN_HEAD + 3 * (size_t)max_append + 1; }
void launch_map_append(hipStream_t st, const MapView& v, const double* xyz, const float* inten, const int64_t* offs, const double* frames,
                       const double* poses, const int* ids, const int* emitted, int N, int64_t max_points, int* info);

// worldmap.hip — the voxel fusion of a map's clouds into one world-frame point set.  WorldMapView: the caller's six
// output buffers, the map's arrays it reads, the create sizes and the scratch of a pr_worldmap (worldmap.cpp), ONE allocation:
//   slots [T][2] u64 (key, representative; cleared to all ones) | cnt [T] i32 | ctl [4] i32 (word 0: the call's flags) (cleared to zero) |
//   slot_of [pcap] i32 (the point's slot, -1: not valid) | blk [2][nblk4] i32 (per 256 points: representatives that qualify, valid points;
//   after the scan the first half holds the exclusive prefix) | the staging of the host form.
// T = the smallest power of two >= max(2 pcap, 64), nblk = ceil(pcap / 256), nblk4 = nblk rounded up to 4.
constexpr int WORLDMAP_OVERFLOW = 1, WORLDMAP_SKIPPED = 2, WORLDMAP_RANGE = 4, WORLDMAP_TABLE = 8;   // = PR_WORLDMAP_*
constexpr int64_t WORLDMAP_MAX_POINTS = (int64_t)1 << 29;      // slot indices and prefixes are int32
struct WorldMapView {
  double* xyz; float* inten; int64_t* src; int* row; int* count; int* state;                // the six output buffers
  const double* m_xyz; const float* m_inten; const int64_t* m_offs; const double* m_poses; const int* m_state;   // the map
  int kcap, log2T, nblk;
  int64_t pcap, ocap;
  unsigned long long* slots; int* cnt; int* ctl; int* slot_of; int* blk;
};
inline int worldmap_log2T(int64_t pcap) { int l = 6; while (((int64_t)1 << l) < 2 * pcap) l++; return l; }
hipError_t launch_worldmap_fuse(hipStream_t st, const WorldMapView& v, const double* poses, const int* n, double cell, int min_count,
                                int keep, int64_t* info);

// maploc.hip — scan-to-map registration against a world map's rows through ONE voxel hash index shared by every pair.
// MapLocView: the three world buffers it reads, the create sizes and the scratch of a pr_maploc (maploc.cpp), ONE allocation:
//   table [T][2] u64 (key, smallest row; cleared to all ones) | ctl [4] i32 (the call's flags, rows indexed; cleared to zero) | offs2 [2]
//   i64 = {0, R} | pair_dst [pair_capacity] i32 zeros | nn_d, nn_j [pair_capacity][ld] | part [pair_capacity][nchunks][ICP_PARTIAL] | done
//   [pair_capacity] | prev [pair_capacity][2] | the staging of the host forms.
// T = the smallest power of two >= max(2 out_capacity, 64), ld = max(max_src_pts, 1), nchunks = ceil(ld / 256).
constexpr int MAPLOC_SKIPPED = 1, MAPLOC_RANGE = 2, MAPLOC_DUPLICATE = 4, MAPLOC_TABLE = 8;          // = PR_MAPLOC_*
constexpr int64_t MAPLOC_MAX_ROWS = (int64_t)1 << 29;
constexpr double MAPLOC_SLACK = 1.0 + 0x1p-10;                   // cell >= max_corr * MAPLOC_SLACK
struct MapLocView {
  const double* xyz; const int* row; const int* state;          // of the world map (caller-owned)
  int64_t ocap;
  double cell;
  int log2T, pair_cap, max_src, ld, nchunks;
  unsigned long long* table; int* ctl; int64_t* offs2; int* pair_dst;
  double* nn_d; int* nn_j; double* part; int* done; double* prev;
};
inline int maploc_log2T(int64_t ocap) { int l = 6; while (((int64_t)1 << l) < 2 * ocap) l++; return l; }
// the target of every pair: the world rows as a one-cloud set
inline IcpClouds maploc_clouds(const MapLocView& v, const double* xyz_q, const int64_t* offs_q, int Nq, const int32_t* pair_src, int c) {
  return IcpClouds{xyz_q, offs_q, Nq, v.xyz, v.offs2, 1, pair_src, v.pair_dst, c, v.max_src, (int)v.ocap};
}
hipError_t launch_maploc_index(hipStream_t st, const MapLocView& v, int64_t* info);
// one pass under T [c][3][4]: results at base[pair] (or pair * ld); excl (or null) [c][2]; done (or null): pairs to skip; part (or null)
// [c][nchunks][ICP_PARTIAL]: the sums of chunks of 256 points (icp_common.hpp's chunk_sums)
void launch_maploc_probe(hipStream_t st, const MapLocView& v, const IcpClouds& A, const double* T, const int32_t* excl, const int* done,
                         const long long* base, double* nn_d, int* nn_j, double mc2, double* part);
void launch_maploc_seed(hipStream_t st, const double* poses, const int* n, int kcap, const int32_t* idx, const unsigned char* accepted,
                        const double* T_rel, const int32_t* src, int c, double* T0, int32_t* pair_src);
// mapplane.hip — world-map normals through the localiser's index and the plane-metric refinement behind its probe.
// A chunk's record: inliers, sum d2, plane correspondents, the 21 entries of sum J J^T (upper triangle, row-major), the 6 of sum J r.
constexpr int MAPPLANE_SUMS = 30;
}  // namespace pr
struct pr_maploc;
namespace pr {
// maploc.cpp: what a pr_mapplane borrows of its localiser (the view's table, sizes and world record; its context)
const MapLocView* maploc_view(pr_maploc* ml);
pr_ctx* maploc_ctx(pr_maploc* ml);
// one lane per row of out_capacity: normals [out_capacity][3], ninfo [out_capacity]; r2 = fl(radius^2)
void launch_mapplane_normals(hipStream_t st, const MapLocView& v, double r2, int min_nbrs, double max_ratio, double* normals, int* ninfo);
// behind launch_maploc_probe with rows at pair * ld: part [c][nchunks][MAPPLANE_SUMS]
void launch_mapplane_sums(hipStream_t st, const IcpClouds& A, const double* T, const int* done, const double* nn_d, const int* nn_j, int ld,
                          int nchunks, double mc2, const double* normals, const int* ninfo, double* part);
void launch_mapplane_update(hipStream_t st, const IcpClouds& A, const double* part, int nchunks, const IcpParams& P, int final_pass, double* T,
                            IcpStats* stats, int* done, double* prev);
}  // namespace pr
struct pr_worldmap;
namespace pr {
// worldmap.cpp: what a pr_mapgrow borrows of its world map (the view's buffers, map arrays and capacities; the map's max_cloud_points;
// its context)
const WorldMapView* worldmap_view(pr_worldmap* wm);
int worldmap_max_cloud(pr_worldmap* wm);
pr_ctx* worldmap_ctx(pr_worldmap* wm);

// mapgrow.hip — the world map, its voxel index and its normals grown by ONE keyframe a call.  MapGrowView: the world
// map's view, the localiser's table and control words, and the scratch of a pr_mapgrow (mapgrow.cpp), ONE allocation:
//   ctl [16] i32 (MAPGROW_* words below) | slot_of [mcp] i32 (the point's slot in the localiser's table, -1: not valid) | blk [2][nblk] i32
//   (per 256 points: representatives of new voxels, valid points; after the scan the first half holds the exclusive prefix) | the staging
//   of the host forms.  mcp = the map's max_cloud_points, nblk = ceil(mcp / 256).
constexpr int MAPGROW_ORDER = 16, MAPGROW_STALE = 32, MAPGROW_FULL = 64;                              // = PR_MAPGROW_*
constexpr int MAPGROW_MAX_CLOUD = 1 << 26;
// ctl words: the handle's four (fused, rows_seen, the last range [a, b)), the call's world-map flags (zero between calls), what the scan
// hands to finish (new voxels, valid points) and the last call's info[3]
constexpr int MG_FUSED = 0, MG_SEEN = 1, MG_A = 2, MG_B = 3, MG_FLAGS = 4, MG_NEW = 5, MG_VALID = 6, MG_LAST = 7;
struct MapGrowView {
  WorldMapView w;                                                 // the six world buffers, the map's arrays, kcap, pcap, ocap
  unsigned long long* table; int* ml_ctl; int64_t* offs2;         // the localiser's
  double cell;
  int log2T, mcp, nblk;
  int* ctl; int* slot_of; int* blk;
};
void launch_mapgrow_sync(hipStream_t st, const MapGrowView& v, const int* n);
// pose_is_row: poses holds the 12 entries of the call's pose row alone (the host form's staging) instead of [keyframe_capacity][12]
void launch_mapgrow_extend(hipStream_t st, const MapGrowView& v, const double* poses, int pose_is_row, const int* row, int64_t* info);
// one lane per (row of the last range, one of the 27 keys around it).  out_rows == NULL: the row a lane recomputes is written at its own
// index of normals / ninfo.  Otherwise lane L writes at L and leaves the row (or -1) in out_rows[L]: the compact form of the host call.
void launch_mapgrow_normals(hipStream_t st, const MapGrowView& v, double r2, int min_nbrs, double max_ratio, double* normals, int* ninfo,
                            int* out_rows);

}  // namespace pr
