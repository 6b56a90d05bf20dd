// dart_amd/csrc/dg_api.hip -- libdartgpu.so: the C ABI of include/dartgpu.h over the HIP kernels.
// gfx950 (MI355X) only; no CPU fallback anywhere: every entry point needs a live HIP device.
#include "../../include/dartgpu.h"
#include "dg_common.h"
#include "dg_fm.h"
#include "dg_seedq.h"
#include "dg_chain.h"
#include "dg_report.h"
#include "dg_pair.h"
#include "dg_reseed.h"
#include "dg_sort.h"
#include "dg_samfmt.h"
#include "dg_bamfmt.h"
#include "dg_bgzf.h"
#include "dg_bgzf_dyn.h"
#include "dg_fastq.h"
#include "dg_trim.h"
#include "dg_inflate.h"
#include "dg_sjtab.h"
#include "dg_bamsort.h"
#include "dg_bamidx.h"
#include "dg_coverage.h"
#include "dg_markdup.h"
#include "dg_umidup.h"
#include "dg_pileup.h"
#include "dg_qc.h"
#include "dg_tags.h"
#include "dg_genecount.h"
#include "dg_rnametrics.h"
#include "dg_txquant.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <algorithm>
#include <vector>
#include <atomic>
#include <mutex>
#include <chrono>
#include <thread>
#include <condition_variable>
#include <fcntl.h>
#include <unistd.h>
#include <sys/stat.h>

static char g_init_error[512] = "";

// A context drives one HIP stream and a host keeps a dozen contexts in flight (dg_clone); the HIP runtime maps every stream of a process
// onto GPU_MAX_HW_QUEUES hardware queues (its default 4), and streams that share a queue run their kernels one after the other.  The
// library needs DG_HW_QUEUES_NEED: twelve contexts + the device's copy stream + the caller's stream + two spare (DESIGN.md 6, round 5,
// item 2).  A value that is missing, unparsable or LOWER than that is raised to it -- a launcher that presets the runtime's default of 4
// must not squeeze twelve contexts onto four queues; a higher value stays (a host that asked for more keeps it).  The variable is read
// when the HIP runtime initialises, so this reaches a host that loads the library before its first HIP call; one that touched HIP first
// exports GPU_MAX_HW_QUEUES itself.  What was found and what was left is kept for dg_init_report and dg_clone.
#define DG_HW_QUEUES_NEED 16
static_assert(DG_HW_QUEUES_NEED <= 32, "more hardware queues than 32 are not asked for");
static char g_hwq_found[24] = "unset";            // the variable's text at load time
static int g_hwq_left = DG_HW_QUEUES_NEED;        // its value when the constructor returned
__attribute__((constructor)) static void dg_default_hw_queues()
{
    const char *v = getenv("GPU_MAX_HW_QUEUES");
    long have = 0;
    if (v) {
        size_t i = 0;
        for (; v[i] && i + 1 < sizeof g_hwq_found; i++) g_hwq_found[i] = (v[i] > ' ' && v[i] < 127 && v[i] != ';' && v[i] != '=') ? v[i] : '?';
        g_hwq_found[i] = 0;
        if (!i) snprintf(g_hwq_found, sizeof g_hwq_found, "empty");
        char *end = nullptr;
        have = strtol(v, &end, 10);
        if (end == v || *end) have = 0; else if (have > 1000000) have = 1000000;
    }
    if (have < DG_HW_QUEUES_NEED) {
        char b[8];
        snprintf(b, sizeof b, "%d", DG_HW_QUEUES_NEED);
        setenv("GPU_MAX_HW_QUEUES", b, 1);
        have = DG_HW_QUEUES_NEED;
    }
    g_hwq_left = (int)have;
}
static std::atomic<int> g_live_ctx[64];           // contexts alive per device (each owns one stream)
static std::atomic<bool> g_hwq_warned{false};

#include "api_ctx.h"

#define N_TIMERS 20
#define N_TOPS 128              // small device counters of a batch (bump tops, tickets, list sizes, class histogram), zeroed per run
enum { TOP_CIG = 0, TOP_SJ, TOP_JOBS, TOP_REPORT_MAIN, TOP_REPORT_JOBS /* reserved, unused */, TOP_HEAVY_UNITS, TOP_SEED_NEXT, TOP_SEED_HEAVY,
       TOP_WORK = 16, TOP_TICKET_PAIR = 17, TOP_TICKET_EMIT = 18, TOP_RESEED_COUNT = 19 /* 19..21: items per ring size; 22: diagonals per chunk */, TOP_RESEED_TICKET = 23 /* 23..25 */, TOP_TICKET_SEED = 26, TOP_RS_POOL = 27, TOP_RS_OUT = 31,
       TOP_ORDER_INFO = 28 /* 28..30 */, TOP_CLASS_HIST = 32 /* 32..63 */, TOP_CLASS_FILL = 64 /* 64..95 */ };        // (explicit values: every index names its own word)

// The index of a device as its contexts see it: the root context owns it, dg_clone()d contexts point to it.  The look-up aids may still be
// under construction when the first batches run (DG_INIT_ASYNC_AIDS): the aids thread publishes a new DIndex (gen + 1) whenever one is
// complete, and every context compares its generation at the start of a run.
struct IndexShared {
    std::mutex mu;
    std::condition_variable cv;
    DIndex ix{};
    std::atomic<uint32_t> gen{1};
    std::thread aids;
    std::atomic<int> aids_state{0};          // 0 = no aids thread, 1 = allocating / building, 2 = complete, -1 = failed (the index works without)
    char aids_msg[256] = "";
    bool upload_done = false, upload_ok = false;
    void *d_ktab = nullptr, *d_sa_dense = nullptr;
    std::string report, report_out;
    int device = 0;
    // chromosome names for the SAM text (dg_set_chr_names): with the index, so every clone prints them
    uint32_t *d_chr_name_off = nullptr; char *d_chr_names = nullptr; bool chr_names_set = false; uint64_t chr_names_gen = 0; uint32_t chr_name_max = 0;
    // the gene annotation's segment table (dg_gene_set_annotation, dg_genecount.h): with the index, so every clone counts with it; gc_gen: 0 = none
    uint32_t *d_gc_chr_first = nullptr, *d_gc_seg_start = nullptr, *d_gc_seg_lab = nullptr; uint32_t gc_n_genes = 0; size_t gc_n_seg = 0; uint64_t gc_gen = 0;
    // the transcript annotation's tables (dg_rna_set_annotation, dg_rnametrics.h): the segment table, the eligible transcripts and their merged exons; rm_gen: 0 = none
    uint32_t *d_rm_chr_first = nullptr, *d_rm_seg_start = nullptr, *d_rm_seg_cs = nullptr; RmTx *d_rm_tx = nullptr; RmExon *d_rm_ex = nullptr;
    size_t rm_n_seg = 0, rm_n_tx = 0, rm_n_elig = 0; uint64_t rm_gen = 0;
    // the expression stage's tables (dg_tx_set_annotation, dg_txquant.h): the segment table with its transcript lists, the transcripts and their merged exons; tx_gen: 0 = none
    uint32_t *d_tx_chr_first = nullptr, *d_tx_seg_start = nullptr, *d_tx_seg_ids = nullptr; uint64_t *d_tx_seg_off = nullptr; TxTx *d_tx_tx = nullptr; TxExon *d_tx_ex = nullptr;
    size_t tx_n_seg = 0; uint32_t tx_n_tx = 0; uint64_t tx_gen = 0;
};

struct dg_ctx {
    int device = 0;
    IndexShared *shared_ix = nullptr; uint32_t ix_gen = 0;
    bool owns_index = true;       // false for dg_clone()d contexts: the index arrays belong to the parent
    hipStream_t stream = nullptr;
    hipEvent_t ev_dl = nullptr, ev_dl_block = nullptr;      // this context's place in the device's copy stream (copy_stream below); _block: the host thread sleeps (DG_BLOCKING_SYNC)
    bool dl_on_copy_stream = false;
    int env_copy_stream = 1;                           // DG_COPY_STREAM: 0 = the downloads on the context's own stream, 1 = on the device's copy stream
    hipEvent_t ev_wait = nullptr;
    char err[512] = "";
    DIndex ix{};
    DParams pr{};
    // index storage (the aids belong to shared_ix)
    void *d_bwt = nullptr, *d_sa = nullptr, *d_pac = nullptr, *d_lockey = nullptr, *d_locchr = nullptr, *d_chroff = nullptr;
    // batch inputs
    int n_reads = 0, max_rlen = 0;
    size_t seq_bytes = 0;
    bool enc_ready = false;       // the packed entry point filled enc itself (no k_encode)
    DBuf<unsigned char> seq; DBuf<uint32_t> seq_off; DBuf<uint16_t> rlen; DBuf<uint32_t> enc; DBuf<uint32_t> packed_in, nlist_in;
    // pipeline buffers; the four whose size depends on the data have sticky capacities (cap_*): a batch is enqueued against
    // them without asking the device for a size first, the device reports what it needed (DSizes) and flags an overflow
    // (d_err >= DG_ABORT), in which case the host grows the buffer and runs the batch again
    DBuf<DHit> hits; DBuf<uint32_t> nhits, nseeds, seed_off, ncand, rep_off, tile_sums, tile_read, slow_units;
    DBuf<SKey> seeds; DBuf<DSeed> work; DBuf<DCand> cands; DBuf<DJob> jobs; DBuf<unsigned long long> job_items, job_pool; DBuf<RsChunkOut> job_outs; DBuf<uint32_t> job_pool_next; DBuf<unsigned long long> items; DBuf<uint32_t> hist, heavy; DBuf<DHeavy> seed_heavy; DBuf<int32_t> seed_heavy_sfail; DBuf<int16_t> chain_picks; DBuf<uint8_t> chain_todo;
    DBuf<dg_read_out> reads_out; DBuf<dg_report_out> reports; DBuf<uint32_t> cigpool, cigfinal;
    DBuf<dg_sj_out> sjpool, sjfinal;
    DBuf<dg_read_c> reads_c; DBuf<dg_report_c> reports_c; DBuf<uint32_t> cig_c;     // compact records and their stored CIGAR ops (written by k_pair / k_emit_slow)
    DBuf<unsigned char> ws;
    DBuf<unsigned long long> scan_state, scan_trace;      // look-back state words / what every tile's workgroup last said about itself (dg_scan.h)
    int wall_khz = 100000;                                // rate of wall_clock64() on this device
    uint32_t scan_epoch = 0;      // number of the enqueued run, carried by every state word of its single-pass scans (dg_scan.h); never 0
    size_t cap_seeds = 0, cap_rep = 0, cap_work = 0, cap_cig = 0;
    // what any context of this index has learned about capacities (the root owns it, clones point to it): a clone does not have to overflow
    // and run its first batch again to find out what its siblings already know
    struct SharedCaps { std::atomic<size_t> seeds{0}, rep{0}, work{0}, cig{0}; } *shared_caps = nullptr;
    bool owns_shared_caps = false;
    unsigned long long *d_ctr = nullptr; unsigned int *d_tops = nullptr; int *d_err = nullptr; DSizes *d_sizes = nullptr; unsigned int *d_input_bad = nullptr;
    struct HostTail { DSizes sizes; int err; unsigned int input_bad; unsigned int tops[N_TOPS]; unsigned long long ctr[CTR_STRIDE]; __host__ __device__ uint32_t *sizes_words() { return (uint32_t *)&sizes; } } *h_tail = nullptr;   // page-locked; written by k_batch_end
    bool state_zeroed = false;   // the small device state (counters, tops, status, sizes) is zero: k_batch_end of the previous run left it so
    size_t used[3] = {0, 0, 0};
    bool enqueued = false;
    // timings
    hipEvent_t ev[N_TIMERS + 1] = {}; const char *tname[N_TIMERS]; int n_t = 0; float tms[N_TIMERS];
    uint64_t counters[CTR_N];
    uint64_t reruns_capacity = 0, reruns_scan = 0;      // since dg_init / dg_clone
    bool want_compact = true, packed_valid = false;     // compact records: written by this run's kernels too / present for the batch that ran last
    bool batch_done = false;       // the batch on the context has been run and waited for
    bool no_batch = false;         // the last upload was a DG_FQ_CHECK_ONLY: there is nothing to run
    // the library stages' state, one struct each (api_ctx.h); every stage's section of this file drives its own
    SamState sam; FqState fq; TrimState tr; InfState inf; BamState bam; SjState sj; BsState bs; BiState bi; CvState cv; MdState md; UdState ud; PuState pu; QcState qc; TgState tg; GcState gc; RmState rm; TxState tx;
    bool want_full = true, full_valid = false;          // the full record types of the units k_pair finishes: written by this run (dg_map_batch_compact does not want them) / present for the batch that ran last
    int n_cu = 256, runs_of_last_batch = 0, attempt_no = 0;
    // environment switches, read once per context (not per batch)
    int env_seed_waves = 4, env_bail_trips = 0 /* 0: 64 trips in k_seed_qf (a trip there is up to three dependent accesses), 128 in the other two */, env_report_bpc = 8, env_no_fast = 0, env_seed_legacy = 0, env_seed_slots_lg = 0, env_seed_wgs = 0, env_blocking_sync = 0;
    int env_seed_phases = 0, env_seed_wg_waves = 4, env_seed_partial = 32, env_seed_multi = 4;   // DG_SEED_PHASES=1: round 2's barrier-phased queue kernel (k_seed_q) instead of the free-running one (k_seed_qf)
    bool seed_qf_used = false;     // the last run's seeding kernel was k_seed_qf (its own-work counters are derived from its slot counts)
    int env_scan_mask = 7;
    int env_chain_bpc = 8, env_seedh_bpc = 8, env_reseed_pct = 100;      // persistent one-wave workgroups per CU of k_chain_heavy / k_seed_heavy; k_reseed's grids in per cent (sweeps: DG_CHAIN_BPC, DG_SEEDH_BPC, DG_RESEED_PCT)
    int env_rs_chunk = RS_CHUNK_DIAGS, env_rs_inline = RS_ENT_INLINE, env_rs_pool = 0;      // test hooks (DG_RS_CHUNK, DG_RS_ENT_MAX, DG_RS_POOL_BLOCKS): diagonals per chunk of a shared re-seeding window, entries a chunk record holds inline, blocks of the entry pool
    int env_scan_budget = 0;      // DG_SCAN_POLL_BUDGET: poll budget of a look-back on the FIRST attempt of a batch (test hook: forces the DG_E_SCAN re-run path)
    // what make_ctx_objects made by hand; every DBuf and every stage above frees itself.  Only dg_destroy deletes a context (device current, stream waited for).
    ~dg_ctx() {
        for (void *p : {(void *)d_ctr, (void *)d_tops, (void *)d_err, (void *)d_sizes, (void *)d_input_bad}) if (p) (void)hipFree(p);
        if (h_tail) (void)hipHostFree(h_tail);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : {ev_wait, ev_dl, ev_dl_block}) if (e) (void)hipEventDestroy(e);
        if (owns_shared_caps) delete shared_caps;
    }
};

static void read_env(dg_ctx *c)
{
    auto geti = [](const char *k, int dflt) { const char *v = getenv(k); return v ? atoi(v) : dflt; };
    c->env_seed_waves = geti("DG_SEED_WAVES", 4); c->env_bail_trips = geti("DG_SEED_BAIL_TRIPS", 0);
    c->env_seed_legacy = geti("DG_SEED_LEGACY", 0); c->env_seed_slots_lg = geti("DG_SEED_SLOTS_LG", 0); c->env_seed_wgs = geti("DG_SEED_WGS", 0); c->env_blocking_sync = geti("DG_BLOCKING_SYNC", 0);
    c->env_report_bpc = geti("DG_REPORT_BPC", 8); c->env_no_fast = geti("DG_NO_FAST_PAIR", 0);
    c->env_scan_budget = geti("DG_SCAN_POLL_BUDGET", 0); c->env_scan_mask = geti("DG_SCAN_POLL_SCANS", 7);
    c->env_seed_phases = geti("DG_SEED_PHASES", 0); c->env_seed_wg_waves = geti("DG_SEED_WG_WAVES", 4); c->env_seed_partial = geti("DG_SEED_PARTIAL_MIN", 32);
    c->env_copy_stream = geti("DG_COPY_STREAM", 1);
    c->env_chain_bpc = std::max(1, geti("DG_CHAIN_BPC", 8)); c->env_seedh_bpc = std::max(1, geti("DG_SEEDH_BPC", 8)); c->env_reseed_pct = std::max(10, geti("DG_RESEED_PCT", 100));
    c->env_rs_chunk = geti("DG_RS_CHUNK", RS_CHUNK_DIAGS); c->env_rs_chunk = std::min(1 << 24, std::max(RS_SUPER, c->env_rs_chunk / RS_SUPER * RS_SUPER));      // (a multiple of the pac super-chunk)
    c->env_rs_inline = std::min(RS_ENT_INLINE, std::max(0, geti("DG_RS_ENT_MAX", RS_ENT_INLINE))); c->env_rs_pool = std::max(0, geti("DG_RS_POOL_BLOCKS", 0));
    c->sam.first_cap = (size_t)std::max(0, geti("DG_SAM_TEXT_FIRST_CAP", 0));
    c->bam.first_cap = (size_t)std::max(0, geti("DG_BAM_FIRST_CAP", 0));
    c->bs.first_cap = (size_t)std::max(0, geti("DG_BAMSORT_FIRST_CAP", 0));
    c->md.hash_bits = geti("DG_MARKDUP_HASH_BITS", MD_HASH_BITS); if (c->md.hash_bits < 1 || c->md.hash_bits > MD_HASH_BITS) c->md.hash_bits = MD_HASH_BITS;
    c->qc.max_groups = geti("DG_QC_MAX_GROUPS", QC_GROUPS); if (c->qc.max_groups < 1 || c->qc.max_groups > QC_GROUPS) c->qc.max_groups = QC_GROUPS;
    c->rm.max_groups = geti("DG_RNA_MAX_GROUPS", RM_GROUPS); if (c->rm.max_groups < 1 || c->rm.max_groups > RM_GROUPS) c->rm.max_groups = RM_GROUPS;
    c->tx.hash_bits = geti("DG_TX_HASH_BITS", 64); if (c->tx.hash_bits < 1 || c->tx.hash_bits > 64) c->tx.hash_bits = 64;
    c->env_seed_multi = geti("DG_SEED_MULTI", 4); if (c->env_seed_multi < 0 || c->env_seed_multi > SQF_MULTI_MAX) c->env_seed_multi = SQF_MULTI_MAX;   // rows of an interval that are located and compared with the text at once (0: single rows only)
}

// a context adopts the aids that were completed since its last run
static inline void refresh_index(dg_ctx *c)
{
    IndexShared *sh = c->shared_ix;
    if (sh && c->ix_gen != sh->gen.load(std::memory_order_acquire)) { std::lock_guard<std::mutex> lk(sh->mu); c->ix = sh->ix; c->ix_gen = sh->gen.load(); }
}

static int fail(dg_ctx *c, int code, const char *what, hipError_t e)
{
    snprintf(c ? c->err : g_init_error, 512, "%s: %s", what, e == hipSuccess ? "error" : hipGetErrorString(e));
    return code;
}
#define HIPCHK(call) do { hipError_t _e = (call); if (_e != hipSuccess) return fail(c, DG_ERR_HIP, #call, _e); } while (0)

// ------------------------------------------------------------------------------------------
// small utility kernels (the sums of the output stages are dg_wgscan.h, the three-launch scan and the sorter's driver dg_sort.h)
// ------------------------------------------------------------------------------------------
// seeds per read -> where every read's seeds start (exclusive scan; seed_off[n] = total, flagged when it exceeds the capacity), the read
// that owns the first seed of every 64-seed tile (k_locate's entry point) and the list of units with more seeds than a lane of k_pair
// holds (k_chain_heavy's work list) -- ONE launch with a single-pass scan (dg_scan.h).  Round 2: three scan launches, k_tile_reads and
// k_heavy_list, each a pass over the 2 M counts.  Thread = 8 consecutive reads (so both mates of a pair are in one thread).
#define SO_PER 8
__global__ void __launch_bounds__(256)
k_seed_offsets(int n_reads, int paired, const uint32_t *__restrict__ nseeds, uint32_t *__restrict__ seed_off, uint32_t *__restrict__ tile_read, uint32_t n_tile_read,
               uint32_t *__restrict__ heavy_list, unsigned int *n_heavy, uint32_t *total_copy, uint32_t cap, TileScan ts, int *err)
{
    __shared__ unsigned long long s_scan[20];
    __shared__ unsigned int s_tile;
    // a status raised before this launch (the seeding kernel's safety net): nseeds cannot be trusted.  DG_E_SEEDS is raised below by the workgroup with the LAST
    // ticket, when every other workgroup is past this line; DG_E_SCAN may come from a look-back of this very launch: the decision is thread 0's (d_tile_ticket_unless)
    const unsigned int tile = d_tile_ticket_unless(ts, &s_tile, threadIdx.x == 0 && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= DG_ABORT);
    if (tile == SCAN_LEAVE) return;
    const uint32_t first = tile * (256u * SO_PER) + threadIdx.x * SO_PER;
    uint32_t v[SO_PER], sum = 0;
    if (first + SO_PER <= (uint32_t)n_reads) {
        const uint4 a = *(const uint4 *)(nseeds + first), b = *(const uint4 *)(nseeds + first + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
        for (int i = 0; i < SO_PER; i++) v[i] = first + i < (uint32_t)n_reads ? nseeds[first + i] : 0u;
    }
#pragma unroll
    for (int i = 0; i < SO_PER; i++) sum += v[i];
    Triple mine, tot;
    mine.x = sum; mine.y = 0; mine.z = 0; mine.w = 0;
    const Triple inb = d_block_exclusive(mine, tot, s_scan);
    const Triple base = d_tile_exclusive(ts, tile, tot, s_scan + 16, err);
    uint32_t run = base.x + inb.x;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < SO_PER; i++) {
        const uint32_t r = first + i;
        if (r < (uint32_t)n_reads) {
            seed_off[r] = run;
            for (uint32_t t = (run + 63u) >> 6; (t << 6) < run + v[i] && t < n_tile_read; t++) tile_read[t] = r;       // (a read with seeds; tiles beyond the capacity: the batch runs again)
        }
        // units with more seeds than k_pair's lanes hold: a pair = reads 2k, 2k+1 of this thread; order of the list is irrelevant
        const bool unit_end = paired ? (i & 1) == 1 : true;
        const uint32_t useeds = paired ? ((i & 1) ? v[i - ((i & 1) ? 1 : 0)] + v[i] : 0u) : v[i];
        const bool heavy = unit_end && r < (uint32_t)n_reads && useeds > (uint32_t)UNIT_MAX_SEEDS;
        const unsigned long long m = __ballot(heavy);
        if (m) {
            unsigned int hb = 0;
            const int leader = __ffsll((long long)m) - 1;
            if (lane == leader) hb = atomicAdd(n_heavy, (unsigned int)__popcll(m));
            hb = (unsigned int)__shfl((int)hb, leader, 64);
            if (heavy) heavy_list[hb + (unsigned int)__popcll(m & ((1ull << lane) - 1ull))] = paired ? r >> 1 : r;
        }
        run += v[i];
    }
    if (tile == gridDim.x - 1 && threadIdx.x == 0) {
        const uint32_t total = base.x + tot.x;
        seed_off[n_reads] = total;
        if (total_copy) *total_copy = total;
        if (total > cap) atomicMax(err, DG_E_SEEDS);       // the consumers of these offsets return at once (DG_ABORT); the host grows the buffer
    }
}

static std::atomic<uint64_t> g_phase_ns[4];
static void caps_publish(std::atomic<size_t> &a, size_t v) { size_t cur = a.load(); while (cur < v && !a.compare_exchange_weak(cur, v)) { } }
static void caps_adopt(size_t &mine, const std::atomic<size_t> &a) { const size_t v = a.load(); if (v > mine) mine = v; }
// waiting for a context's stream on the per-batch path.  DG_BLOCKING_SYNC=1: through an event created with hipEventBlockingSync, so the
// host thread sleeps instead of spinning (one thread per context: a dozen spinning threads per GPU is a dozen busy cores)
// One copy stream per device, with the highest priority, shared by all contexts of the device (dg_clone), for the downloads.  A context's
// download is four copies; on its own stream each of them is a blit launch that queues among a dozen batches' kernels (a third of a
// context's cycle was spent there).  On the device's copy stream they run ahead of the kernels and one batch after the other: 853
// against 797-838 M reads/s (profiles/r03/h_copy_stream.txt).  One such stream PER CONTEXT is far worse (621): too many queues; the
// uploads on a stream of the same kind (the context's stream waiting for an event): 827 against 850.
// The host has waited for the run before it downloads, so the copy stream needs no dependency on the context's stream; the context waits
// for its own event behind its copies.  The streams live as long as the process.
static std::mutex g_copy_mu[64];
static hipStream_t g_copy_stream[64][2];
static hipError_t copy_stream(int device, int dir, hipStream_t *out)
{
    hipStream_t &sl = g_copy_stream[device & 63][dir];
    if (!sl) {
        int lo = 0, hi = 0;
        hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&sl, hipStreamNonBlocking, hi);
        if (e != hipSuccess) { sl = nullptr; return e; }
    }
    *out = sl;
    return hipSuccess;
}

// The shared copy stream pays off for page-locked destinations (true asynchronous DMA).  A copy into ordinary memory is staged and blocks its caller --
// under the device-wide mutex every other context's download would wait behind it (`dart`'s streaming path passes ordinary arrays): those go
// through the context's own stream.
static bool host_page_locked(const void *p)
{
    if (!p) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

static hipError_t wait_stream(dg_ctx *c)
{
    if (!c->env_blocking_sync || !c->ev_wait) return hipStreamSynchronize(c->stream);
    const hipError_t e = hipEventRecord(c->ev_wait, c->stream);
    return e != hipSuccess ? e : hipEventSynchronize(c->ev_wait);
}

// ------------------------------------------------------------------------------------------
// k_report: persistent waves; one lane = one read at a time (GenMappingReport,
// AlignmentCandidates.cpp:1079-1207); results go to the read's dg_read_out / dg_report_out slots
// ------------------------------------------------------------------------------------------
#ifdef DG_PROFILE_CLASSES          // diagnostic build only (profiles/probes/class_profile.sh): shader cycles per cost class
__device__ unsigned long long g_class_cycles[DG_COST_CLASSES + 1], g_class_chunks[DG_COST_CLASSES + 1];
#endif
template <int MINW>
__global__ void __launch_bounds__(64, MINW)
k_report(const DIndex ix, const DParams pr, int n_reads, int paired, const unsigned char *__restrict__ seq,
         const uint32_t *__restrict__ seq_off, const uint16_t *__restrict__ rlen, const uint32_t *__restrict__ seed_off,
         const DJob *__restrict__ jobs, DCand *__restrict__ cands,
         const uint32_t *__restrict__ rep_off, DSeed *__restrict__ work, const unsigned long long *__restrict__ items,
         const uint32_t *__restrict__ n_items_p, dg_report_out *__restrict__ reports, uint32_t *cigpool, uint32_t cigcap,
         unsigned int *tops, unsigned char *ws, const WSLayout L, unsigned long long *ctr, int *err)
{
    const unsigned long long t_wave0 = wall_clock64();
    const int lane = blockIdx.x * blockDim.x + threadIdx.x;
    __shared__ uint32_t lds_pm[64 * PM_LDS_WORDS];
    if (*err >= DG_ABORT) return;
    LaneCtx cx;
#ifdef DG_PROFILE_CLASSES
    __shared__ unsigned long long ph_acc[DG_NCLS * DG_NPHASE], cls_acc[2 * DG_NCLS];
    for (int q = threadIdx.x; q < DG_NCLS * DG_NPHASE; q += 64) ph_acc[q] = 0;
    for (int q = threadIdx.x; q < 2 * DG_NCLS; q += 64) cls_acc[q] = 0;
    __syncthreads();
    cx.ph = ph_acc;
#endif
    cx.lds = lds_pm + (threadIdx.x & 63) * PM_LDS_WORDS;
    cx.ix = &ix; cx.pr = &pr; cx.L = &L;
    cx.ws = ws + (size_t)lane * L.stride;
    cx.n_nw = cx.nw_cells = cx.n_reseed = cx.reseed_w = 0;
    // items = [candidates that waited for k_reseed | all other live candidates of the listed reads, heaviest class first] (k_order_items); this launch takes
    // the whole list (k_reseed has run), 64 items per ticket: lane = candidate.  (Rounds 1-4: lane = read, and the reads with dozens of candidates a wave each.)
    const unsigned int lo = 0u, hi = *n_items_p;
    unsigned int *next = tops + TOP_REPORT_MAIN;
    while (true) {
        unsigned int ticket = 0;
        if ((threadIdx.x & 63) == 0) ticket = atomicAdd(next, 1u);
        ticket = (unsigned int)__shfl((int)ticket, 0, 64);
        const unsigned int base = lo + ticket * 64u;
        if (base >= hi) break;
        const unsigned int idx = base + (threadIdx.x & 63);
        const bool valid = idx < hi;                               // every lane enters d_gen_mapping_report (it has wave-wide steps)
        const unsigned long long item = valid ? items[idx] : 0ull;
        const int r = (int)(item >> 32);
        const uint32_t ci = (uint32_t)item, rep_i = valid ? rep_off[r] + (ci - seed_off[r]) : 0u;
        DRead rd;
        rd.sub_score = 0; rd.mis_num = 0; rd.mapq = 0;
        cx.seq = seq + seq_off[r]; cx.rlen = rlen[r];
#ifdef DG_PROFILE_CLASSES
        const long long t_begin = clock64();
        cx.cls = (int)(cands[(uint32_t)items[base]].final_n & 31); cx.t_last = t_begin;
#endif
        d_gen_mapping_report(cx, valid, paired ? (r & 1) == 0 : true, rd, cands + ci, valid ? 1 : 0, jobs, work,
                             reports + rep_i, rep_i, cigpool, tops + 0, cigcap, err, 0, 1, true);
#ifdef DG_PROFILE_CLASSES
        if ((threadIdx.x & 63) == 0) { cls_acc[cx.cls] += (unsigned long long)(clock64() - t_begin); cls_acc[DG_NCLS + cx.cls] += 1ull; }
#endif
    }
#ifdef DG_PROFILE_CLASSES
    __syncthreads();
    for (int q = threadIdx.x; q < DG_NCLS * DG_NPHASE; q += 64) if (ph_acc[q]) atomicAdd(&g_phase[q / DG_NPHASE][q % DG_NPHASE], ph_acc[q]);
    if (threadIdx.x < DG_NCLS && cls_acc[DG_NCLS + threadIdx.x]) { atomicAdd(&g_class_cycles[threadIdx.x], cls_acc[threadIdx.x]); atomicAdd(&g_class_chunks[threadIdx.x], cls_acc[DG_NCLS + threadIdx.x]); }
#endif
    d_wave_add(ctr + CTR_NW, cx.n_nw);
    d_wave_add(ctr + CTR_NWCELLS, cx.nw_cells);
    d_wave_add(ctr + CTR_RESEED, cx.n_reseed);
    d_wave_add(ctr + CTR_RESEEDW, cx.reseed_w);
    d_wave_resident(ctr, CTR_WT_REPORT, t_wave0);
}

// ------------------------------------------------------------------------------------------
// k_finalize: one lane = one unit of the general path (slow_units[]): CheckPairedFinalAlignments, FLAGs, MAPQ,
// splice-junction tuples (Mapping.cpp:74-206,479-565,615-621) on the records k_report left in memory
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_finalize(const DIndex ix, const DParams pr, int paired, const uint32_t *__restrict__ slow_units, const DSizes *__restrict__ sizes,
           const uint32_t *__restrict__ seed_off, const DCand *__restrict__ cands, const uint32_t *__restrict__ ncand, const uint32_t *__restrict__ rep_off, const DSeed *__restrict__ work,
           dg_read_out *__restrict__ rout, dg_report_out *__restrict__ reports, dg_sj_out *sjpool, uint32_t sjcap, unsigned int *tops, int *err)
{
    if (*err >= DG_ABORT) return;
    const unsigned int n_units = sizes->n_slow_units;
    for (unsigned int it = blockIdx.x * blockDim.x + threadIdx.x; it < n_units; it += gridDim.x * blockDim.x) {
        const int u = (int)slow_units[it];
        const int nm = paired ? 2 : 1;
        DRead rd[2];
        dg_read_out o[2];
        RepMem<dg_report_out> rp[2];
        for (int m = 0; m < nm; m++) {
            const int r = paired ? 2 * u + m : u;
            const int nc = (int)ncand[r];
            dg_report_out *rep = reports + rep_off[r];
            // the running best / second best of GenMappingReport :1161-1172, in candidate order, over what k_report's lanes (one candidate each) left:
            // aln_score, and the candidate's mismatch count parked in `flag`.  SURVEY F6: sub_score, mis_num, mapq start at 0
            rd[m].score = 0; rd[m].sub_score = 0; rd[m].mis_num = 0; rd[m].mapq = 0; rd[m].iBest = 0; rd[m].CanNum = nc > 0 ? nc : 1;
            for (int i = 0; i < nc; i++) {
                const int aln = rep[i].aln_score, mis_num = rep[i].flag;
                if (mis_num) rep[i].flag = 0;                       // (also where the reference zeroes aln late, :1157: the parked value must not stay)
                if (aln <= 0) continue;                            // such an aln changes nothing: score and sub_score are 0 or stay
                if (aln > rd[m].score) { rd[m].iBest = i; rd[m].mis_num = mis_num; rd[m].sub_score = rd[m].score; rd[m].score = aln; }
                else if (aln == rd[m].score) rd[m].sub_score = rd[m].score;
            }
            o[m].score = rd[m].score; o[m].sub_score = rd[m].sub_score; o[m].mis_num = rd[m].mis_num; o[m].mapq = 0;
            o[m].n_rep = rd[m].CanNum; o[m].best = rd[m].iBest; o[m].rep_off = (int32_t)rep_off[r]; o[m].sj_off = 0; o[m].n_sj = 0;
            rp[m].p = rep;
        }
        if (paired) {
            d_settle_pair(pr, rd[0], rp[0], rd[1], rp[1]);
            d_flag_pair(rd[0], rp[0], rd[1], rp[1]);
        } else d_flag_single(rd[0], rp[0]);
        for (int m = 0; m < nm; m++) {
            const int r = paired ? 2 * u + m : u;
            d_mapq(rd[m], rp[m]);
            o[m].score = rd[m].score; o[m].mapq = rd[m].mapq; o[m].best = rd[m].iBest;
            if (ncand[r] > 0 && (rd[m].mapq == 50 || (pr.all_sj && rd[m].score > 0)))
                d_collect_sj(ix, pr, cands[seed_off[r] + rd[m].iBest], work, r, sjpool, tops + TOP_SJ, sjcap, o[m].sj_off, o[m].n_sj, err);
            rout[r] = o[m];
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_emit_slow: the variable-length records of the general path's reads, laid out deterministically behind k_pair's: one lane
// = one read of slow_units[] (ascending); a single-pass scan (dg_scan.h) of (CIGAR ops, junction tuples) per read gives the
// places; CIGAR ops move from the report kernel's pool to cigfinal[cig_fast + ...], tuples from the bump pool to sjfinal.
// The grid covers the worst case (every unit on the list); workgroups beyond the list leave at once.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_emit_slow(int paired, const uint32_t *__restrict__ slow_units, DSizes *sizes, dg_read_out *__restrict__ rout, dg_report_out *__restrict__ reports,
            const uint32_t *__restrict__ cigpool, uint32_t *__restrict__ cigfinal, uint32_t cap_cig, const dg_sj_out *__restrict__ sjpool, dg_sj_out *__restrict__ sjfinal,
            TileScan ts, int *err, const uint16_t *__restrict__ rlen, const CompactOut co)
{
    __shared__ unsigned long long s_scan[20];
    __shared__ unsigned int s_tile;
    bool leave = false;                                           // (DG_E_CIGFINAL may have been raised by an earlier workgroup of this launch; thread 0 decides for the workgroup)
    if (threadIdx.x == 0) { const int e0 = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); leave = e0 >= DG_ABORT && e0 != DG_E_CIGFINAL; }
    const unsigned int tile = d_tile_ticket_unless(ts, &s_tile, leave);
    if (tile == SCAN_LEAVE) return;
    const unsigned int n_items = sizes->n_slow_units * (paired ? 2u : 1u);
    if (tile > 0 && tile * 256u >= n_items) return;
    const unsigned int it = tile * 256u + threadIdx.x;
    const bool on = it < n_items;
    const int r = on ? (paired ? (int)(2u * slow_units[it >> 1] + (it & 1u)) : (int)slow_units[it]) : 0;
    dg_read_out o;
    o.n_rep = 0; o.rep_off = 0; o.n_sj = 0; o.sj_off = 0;
    if (on) o = rout[r];
    uint32_t ncig = 0, ncigc = 0;
    const uint32_t full_match = on ? (uint32_t)rlen[r] << 4 : 0u;                      // "<rlen>M": not stored in the compact op array
    for (int i = 0; i < (on ? o.n_rep : 0); i++) {
        const dg_report_out &rp = reports[o.rep_off + i];
        ncig += rp.n_cigar;
        if (co.reads) ncigc += (rp.n_cigar == 1u && cigpool[rp.cigar_off] == full_match) ? 0u : rp.n_cigar;
    }
    Triple mine, tot;
    mine.x = ncig; mine.y = on ? (uint32_t)o.n_sj : 0u; mine.z = 0; mine.w = ncigc;
    const Triple inb = d_block_exclusive(mine, tot, s_scan);
    const Triple base = d_tile_exclusive(ts, tile, tot, s_scan + 16, err);
    const uint32_t cig_fast = sizes->cig_fast, cigc_fast = sizes->pad[2];
    if (on) {
        uint32_t dst = cig_fast + base.x + inb.x, dstc = cigc_fast + base.w + inb.w;
        bool fits = true;
        if ((uint64_t)dst + ncig > cap_cig) atomicMax(err, DG_E_CIGFINAL);
        else for (int i = 0; i < o.n_rep; i++) {
            dg_report_out &rp = reports[o.rep_off + i];
            const uint32_t m = rp.n_cigar, src = rp.cigar_off;
            const bool plain = m == 1u && cigpool[src] == full_match;
            for (uint32_t k = 0; k < m; k++) cigfinal[dst + k] = cigpool[src + k];
            if (co.reads) {                                        // the compact form of the same report; its stored ops lie in the op array's second region
                if (!plain) { for (uint32_t k = 0; k < m; k++) co.cigar[dstc + k] = cigpool[src + k]; dstc += m; }
                dg_report_c q; fits = d_compact_report(rp, plain, true, q) && fits; co.reports[o.rep_off + i] = q;
            }
            rp.cigar_off = dst; dst += m;
        }
        if (o.n_sj > 0) {
            const uint32_t sd = base.y + inb.y;
            for (int k = 0; k < o.n_sj; k++) sjfinal[sd + k] = sjpool[o.sj_off + k];
            rout[r].sj_off = (int32_t)sd;
        }
        if (co.reads) { dg_read_c oc; fits = d_compact_read(o, oc) && fits; co.reads[r] = oc; if (!fits) *co.bad = 1u; }
    }
    const unsigned int last = n_items ? (n_items - 1u) / 256u : 0u;
    if (tile == last && threadIdx.x == 0) { sizes->total_cig = cig_fast + base.x + tot.x; sizes->total_sj = base.y + tot.y; sizes->pad[0] = cigc_fast + base.w + tot.w; }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
extern "C" void dg_params_default(dg_params *p)
{
    p->max_gaps = 5; p->max_dup = 100; p->max_intron = 500000; p->min_intron = 5;
    p->max_mismatch = 0; p->multi_hit = 0; p->all_sj = 0; p->paired = 0;
}

static void set_params(dg_ctx *c, const dg_params *p)
{
    c->pr.max_gaps = p->max_gaps; c->pr.max_dup = p->max_dup; c->pr.max_intron = p->max_intron; c->pr.min_intron = p->min_intron;
    c->pr.max_mismatch = p->max_mismatch; c->pr.multi_hit = p->multi_hit; c->pr.all_sj = p->all_sj; c->pr.paired = p->paired;
}

extern "C" int dg_set_params(dg_ctx *c, const dg_params *p)
{
    if (!c || !p) return DG_ERR_ARG;
    set_params(c, p);
    read_env(c);                    // the DG_* tuning switches are read here and at init, never per batch
    return DG_OK;
}

extern "C" int dg_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

extern "C" const char *dg_last_error(const dg_ctx *c) { return c ? c->err : g_init_error; }

extern "C" void dg_destroy(dg_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->owns_index && c->shared_ix) {          // the aids thread may still be allocating or building: it ends by itself (a failed upload tells it so)
        IndexShared *sh = c->shared_ix;
        { std::lock_guard<std::mutex> lk(sh->mu); if (!sh->upload_done) { sh->upload_done = true; sh->upload_ok = false; } }
        sh->cv.notify_all();
        if (sh->aids.joinable()) sh->aids.join();
        if (sh->d_ktab) (void)hipFree(sh->d_ktab);
        if (sh->d_sa_dense) (void)hipFree(sh->d_sa_dense);
        if (sh->d_chr_name_off) (void)hipFree(sh->d_chr_name_off);
        if (sh->d_chr_names) (void)hipFree(sh->d_chr_names);
        for (void *p : {(void *)sh->d_gc_chr_first, (void *)sh->d_gc_seg_start, (void *)sh->d_gc_seg_lab}) if (p) (void)hipFree(p);
        for (void *p : {(void *)sh->d_rm_chr_first, (void *)sh->d_rm_seg_start, (void *)sh->d_rm_seg_cs, (void *)sh->d_rm_tx, (void *)sh->d_rm_ex}) if (p) (void)hipFree(p);
        for (void *p : {(void *)sh->d_tx_chr_first, (void *)sh->d_tx_seg_start, (void *)sh->d_tx_seg_ids, (void *)sh->d_tx_seg_off, (void *)sh->d_tx_tx, (void *)sh->d_tx_ex}) if (p) (void)hipFree(p);
        delete sh; c->shared_ix = nullptr;
    }
    void *ptrs[] = { c->d_bwt, c->d_sa, c->d_pac, c->d_lockey, c->d_locchr, c->d_chroff };
    if (c->owns_index) for (void *p : ptrs) if (p) (void)hipFree(p);
    if (c->stream) { (void)hipStreamDestroy(c->stream); g_live_ctx[c->device & 63].fetch_sub(1); }
    delete c;                      // everything else the context owns frees itself (api_ctx.h): the device is current, the stream has been waited for
}

// per-context objects that dg_init and dg_clone both need
static hipError_t make_ctx_objects(dg_ctx *c)
{
    hipError_t e;
    if ((e = hipStreamCreate(&c->stream)) != hipSuccess) return e;
    g_live_ctx[c->device & 63].fetch_add(1);
    if ((e = hipEventCreateWithFlags(&c->ev_wait, hipEventBlockingSync | hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_dl, hipEventDisableTiming)) != hipSuccess || (e = hipEventCreateWithFlags(&c->ev_dl_block, hipEventBlockingSync | hipEventDisableTiming)) != hipSuccess) return e;
    for (int i = 0; i <= N_TIMERS; i++) if ((e = hipEventCreate(&c->ev[i])) != hipSuccess) return e;
    if ((e = hipMalloc((void **)&c->d_ctr, CTR_STRIPES * CTR_STRIDE * 8)) != hipSuccess || (e = hipMalloc((void **)&c->d_tops, N_TOPS * 4)) != hipSuccess ||
        (e = hipMalloc((void **)&c->d_err, 4)) != hipSuccess || (e = hipMalloc((void **)&c->d_sizes, sizeof(DSizes))) != hipSuccess ||
        (e = hipMalloc((void **)&c->d_input_bad, 4)) != hipSuccess) return e;
    if ((e = hipHostMalloc((void **)&c->h_tail, sizeof(dg_ctx::HostTail), hipHostMallocDefault)) != hipSuccess) return e;
    memset(c->h_tail, 0, sizeof(dg_ctx::HostTail));
    { int khz = 0; if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) == hipSuccess && khz > 0) c->wall_khz = khz; }
    read_env(c);
    return hipSuccess;
}

// ------------------------------------------------------------------------------------------
// start-up: index bytes -> HBM through page-locked staging chunks, look-up aids built beside (or behind) it
// ------------------------------------------------------------------------------------------
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// where a chunk's bytes come from: a file (pread: page cache -> staging chunk) or the caller's host array (memcpy)
struct UpSrc { int fd = -1; const uint8_t *mem = nullptr; };
struct UpChunk { UpSrc src; uint64_t src_off; uint8_t *dst; size_t bytes; uint64_t relayout_blocks; };

// Reader threads take chunks in order; each owns a copy stream and two page-locked staging buffers, so a chunk's read from the page
// cache overlaps the previous chunk's DMA, and the threads' reads overlap each other (one thread copies ~4 GB/s out of the page cache;
// the link takes 50).  The Occ blocks of a .bwt chunk are re-laid in place on the same stream, behind the chunk's copy.
static hipError_t upload_chunks(int device, const std::vector<UpChunk> &chunks, size_t chunk_cap, int n_threads, std::string &what)
{
    std::atomic<size_t> next{0};
    std::atomic<int> failed{0};
    std::mutex mu;
    hipError_t first = hipSuccess;
    auto fail_with = [&](hipError_t e, const char *w) { std::lock_guard<std::mutex> lk(mu); if (!failed.exchange(1)) { first = e == hipSuccess ? hipErrorUnknown : e; what = w; } };
    auto work = [&]() {
        hipError_t e;
        if ((e = hipSetDevice(device)) != hipSuccess) { fail_with(e, "hipSetDevice (index upload)"); return; }
        hipStream_t s = nullptr; uint8_t *pin[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr}; bool used[2] = {false, false};
        if ((e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess) { fail_with(e, "hipStreamCreate (index upload)"); return; }
        for (int b = 0; b < 2 && e == hipSuccess; b++) {
            if ((e = hipHostMalloc((void **)&pin[b], chunk_cap, hipHostMallocDefault)) == hipSuccess) e = hipEventCreateWithFlags(&ev[b], hipEventDisableTiming);
        }
        if (e != hipSuccess) fail_with(e, "page-locked staging buffers (index upload)");
        int b = 0;
        while (e == hipSuccess && !failed.load()) {
            const size_t i = next.fetch_add(1);
            if (i >= chunks.size()) break;
            const UpChunk &ch = chunks[i];
            if (used[b] && (e = hipEventSynchronize(ev[b])) != hipSuccess) { fail_with(e, "hipEventSynchronize (index upload)"); break; }
            if (ch.src.mem) memcpy(pin[b], ch.src.mem + ch.src_off, ch.bytes);
            else {
                size_t got = 0;
                while (got < ch.bytes) {
                    const ssize_t r = pread(ch.src.fd, pin[b] + got, ch.bytes - got, (off_t)(ch.src_off + got));
                    if (r <= 0) break;
                    got += (size_t)r;
                }
                if (got < ch.bytes) { fail_with(hipErrorUnknown, "an index file is shorter than its header says"); break; }
            }
            if (ch.bytes && (e = hipMemcpyAsync(ch.dst, pin[b], ch.bytes, hipMemcpyHostToDevice, s)) != hipSuccess) { fail_with(e, "hipMemcpyAsync (index upload)"); break; }
            if (ch.relayout_blocks) {
                k_relayout_bwt<<<(unsigned)((ch.relayout_blocks + 255) / 256), 256, 0, s>>>((uint4 *)ch.dst, ch.relayout_blocks);
                if ((e = hipGetLastError()) != hipSuccess) { fail_with(e, "k_relayout_bwt"); break; }
            }
            if ((e = hipEventRecord(ev[b], s)) != hipSuccess) { fail_with(e, "hipEventRecord (index upload)"); break; }
            used[b] = true; b ^= 1;
        }
        if (s && (e = hipStreamSynchronize(s)) != hipSuccess) fail_with(e, "index upload");
        for (int k = 0; k < 2; k++) { if (ev[k]) (void)hipEventDestroy(ev[k]); if (pin[k]) (void)hipHostFree(pin[k]); }
        if (s) (void)hipStreamDestroy(s);
    };
    std::vector<std::thread> th;
    for (int t = 0; t < n_threads; t++) th.emplace_back(work);
    for (auto &t : th) t.join();
    return failed.load() ? first : hipSuccess;
}

static void add_chunks(std::vector<UpChunk> &out, UpSrc src, uint64_t src_off, uint8_t *dst, size_t bytes, size_t chunk, bool relayout, uint64_t total_blocks)
{
    for (size_t o = 0; o < bytes || (relayout && o / 64 < total_blocks); o += chunk) {
        const size_t nb = o < bytes ? std::min(chunk, bytes - o) : 0;
        uint64_t rb = 0;
        if (relayout) { const uint64_t first = o / 64; rb = std::min<uint64_t>(chunk / 64, total_blocks > first ? total_blocks - first : 0); }
        out.push_back(UpChunk{src, src_off + o, dst + o, nb, rb});
    }
}

// the look-up aids (full suffix array, K-mer prefix table): allocated while the index loads, built once it is in HBM, on a stream of the
// lowest priority so that batches already being mapped (DG_INIT_ASYNC_AIDS) keep the GPU.  Each aid is published when complete.
static void aids_thread(IndexShared *sh, int sa_file_intv, uint64_t n_sa, bool async, uint64_t expected_reads)
{
    auto failed = [&](const char *w, hipError_t e) {
        std::lock_guard<std::mutex> lk(sh->mu);
        snprintf(sh->aids_msg, sizeof sh->aids_msg, "%s: %s", w, hipGetErrorString(e));
        sh->aids_state.store(-1); sh->cv.notify_all();
    };
    hipError_t e;
    if ((e = hipSetDevice(sh->device)) != hipSuccess) return failed("hipSetDevice (aids)", e);
    DIndex ix;
    { std::lock_guard<std::mutex> lk(sh->mu); ix = sh->ix; }
    const uint64_t seq_len = ix.seq_len;
    double t0 = now_s();
    // full suffix array (8 bytes per text symbol: 1 GB for chr20, 50 GB for a human genome -- this is what 288 GB are for): locating a row is
    // one load instead of a walk of up to 31 LF steps.  Texts too large for that fall back to every 2nd / 4th row; DG_SA_DENSE=0 turns it
    // off, =2/4/8/16 forces an interval
    // A job known to be short (dg_index_files::expected_reads) gets LEAN aids -- every 4th row of the SA and K <= 14: 17 GB instead of 118 GB for
    // a human genome, the seeding stage twice as long (1.85 + 0.25 against 0.97 + 0.10 ms per 2 M reads, profiles/r04/b_init_probe_aids_vs_startup.txt)
    // -- because the full ones cost more than they save below some hundred million reads: 0.7 s of build kernels, and up to 3-4 s of hipMalloc
    // when the device's memory was in use a moment ago (the driver clears VRAM behind a release; an allocation that needs those pages waits).
    const bool lean = expected_reads != 0 && expected_reads < 400000000ull;
    int intv = seq_len <= (12ull << 30) ? 1 : (seq_len <= (24ull << 30) ? 2 : 4);
    if (lean && intv < 4) intv = 4;
    if (const char *v = getenv("DG_SA_DENSE")) intv = atoi(v);
    const bool want_dense = intv >= 1 && intv < sa_file_intv && (intv & (intv - 1)) == 0 && seq_len < (1ull << 39);
    const uint64_t n_entries = want_dense ? seq_len / (uint64_t)intv + 1 : 0;
    int K = 8;
    while (K < 16 && (1ull << (2 * K)) < seq_len) K++;
    if (lean && K > 14) K = 14;
    if (async) {
        // the caller maps batches meanwhile: the device allocations below take a lock every other allocation of the process needs (a context's
        // first batch sizes its buffers) and, on recently used memory, seconds -- so they start only when the index itself is in HBM
        std::unique_lock<std::mutex> lk(sh->mu);
        sh->cv.wait(lk, [&]() { return sh->upload_done; });
        if (!sh->upload_ok) { lk.unlock(); sh->aids_state.store(-1); sh->cv.notify_all(); return; }
    }
    if (want_dense && (e = hipMalloc(&sh->d_sa_dense, n_entries * 8)) != hipSuccess) return failed("hipMalloc dense SA", e);
    // K-mer prefix table: the smallest K with 4^K >= text length (so that most K-mers are unique or absent and a search needs the table plus
    // a step or two), 8 <= K <= 16: 16 bytes per entry = 4.3 GB at K = 14 (chr20), 69 GB at K = 16 (human; K = 14: k_seed 1.31 instead of
    // 0.97 ms).  DG_KTAB_K=0 turns it off, =2..16 forces K.
    {   // the table must leave room for the batches in flight: step down while it would not leave 48 GB free
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            while (K > 8 && ((size_t)16 << (2 * K)) + ((size_t)48 << 30) > free_b) K--;
    }
    if (const char *v = getenv("DG_KTAB_K")) K = atoi(v);
    if (K > 16) K = 16;
    if (K >= 2 && (e = hipMalloc(&sh->d_ktab, ((size_t)16) << (2 * K))) != hipSuccess) return failed("hipMalloc k-mer table", e);
    const double t_alloc = now_s() - t0;
    int lo = 0, hi = 0;
    hipStream_t s = nullptr;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);                    // (lo = the least priority)
    if ((e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, lo)) != hipSuccess) return failed("hipStreamCreate (aids)", e);
    {   // wait for the index bytes
        std::unique_lock<std::mutex> lk(sh->mu);
        sh->cv.wait(lk, [&]() { return sh->upload_done; });
        if (!sh->upload_ok) { lk.unlock(); (void)hipStreamDestroy(s); sh->aids_state.store(-1); sh->cv.notify_all(); return; }
    }
    double t_dense = 0, t_ktab = 0;
    // Built beside running batches (async), the two kernels take a quarter of the wave slots (4 workgroups of 256 per CU, grid-stride): the
    // stream's low priority alone did not keep them from crowding the batches out (a batch waited for the whole build, profiles/r04/a_*).
    int n_cu = 256;
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, sh->device) == hipSuccess && prop.multiProcessorCount > 0) n_cu = prop.multiProcessorCount; }
    int per_cu = 4;
    if (const char *v = getenv("DG_AIDS_WGS_PER_CU")) per_cu = std::max(1, atoi(v));
    const uint64_t grid_cap = async ? (uint64_t)n_cu * (uint64_t)per_cu : (uint64_t)1 << 22;
    if (want_dense) {
        t0 = now_s();
        k_build_sa_dense<<<(unsigned)std::min<uint64_t>((n_sa + 255) / 256, grid_cap), 256, 0, s>>>(ix, intv, n_entries, (uint64_t *)sh->d_sa_dense);
        if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(s)) != hipSuccess) { (void)hipStreamDestroy(s); return failed("k_build_sa_dense", e); }
        ix.sa_dense = (const uint64_t *)sh->d_sa_dense; ix.sa_dense_intv = intv; ix.sa_dense_shift = 0;
        for (int b = 0; (1 << b) < intv; b++) ix.sa_dense_shift = b + 1;
        { std::lock_guard<std::mutex> lk(sh->mu); sh->ix = ix; sh->gen.fetch_add(1, std::memory_order_release); }
        t_dense = now_s() - t0;
    }
    if (K >= 2) {
        t0 = now_s();
        const size_t entries = (size_t)1 << (2 * K);
        k_build_ktab<<<(unsigned)std::min<uint64_t>((entries + 255) / 256, grid_cap), 256, 0, s>>>(ix, K, (uint64_t *)sh->d_ktab);
        if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(s)) != hipSuccess) { (void)hipStreamDestroy(s); return failed("k_build_ktab", e); }
        ix.ktab = (const uint64_t *)sh->d_ktab; ix.ktab_k = K;
        { std::lock_guard<std::mutex> lk(sh->mu); sh->ix = ix; sh->gen.fetch_add(1, std::memory_order_release); }
        t_ktab = now_s() - t0;
    }
    (void)hipStreamDestroy(s);
    {
        std::lock_guard<std::mutex> lk(sh->mu);
        char b[256];
        snprintf(b, sizeof b, "; %saids%s: hipMalloc %.3f s (full SA every %d row(s) %.1f GB, K=%d table %.1f GB), k_build_sa_dense %.3f s, k_build_ktab %.3f s",
                 lean ? "lean " : "", async ? " (built beside the first batches)" : "", t_alloc, want_dense ? intv : 0, n_entries * 8 / 1e9, K >= 2 ? K : 0, K >= 2 ? (double)((size_t)16 << (2 * K)) / 1e9 : 0.0, t_dense, t_ktab);
        sh->report += b;
        sh->aids_state.store(2);
    }
    sh->cv.notify_all();
}

// The second strand of the text, once per index: pac arrives as the forward half (PREFIX.pac, or the caller's array) and leaves dg_init* as all 2L symbols,
// so that no kernel computes a reverse complement per access (d_pac_both, dg_common.h).  Thread = output byte, from the byte that holds symbol L on; that
// byte is composed of forward symbols and the first reverse ones when L is no multiple of 4.
__global__ void __launch_bounds__(256)
k_pac_both(uint8_t *pac, int64_t L, int64_t first_byte, int64_t n_bytes)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_bytes) pac[first_byte + i] = d_pac_both_byte(pac, L, first_byte + i);
}
static size_t pac_both_bytes(int64_t L) { return (size_t)((2 * L + 3) / 4); }
static hipError_t pac_fill_second_half(uint8_t *d_pac, int64_t L, hipStream_t s)
{
    const int64_t first = L / 4, n = (int64_t)pac_both_bytes(L) - first;
    if (n <= 0) return hipSuccess;
    k_pac_both<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_pac, L, first, n);
    hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : hipStreamSynchronize(s);
}

struct IndexMeta { uint64_t bwt_words, primary, L2[5], seq_len, n_sa; int sa_intv; int64_t l_pac; int n_chr; const int64_t *chr_off, *chr_len; uint64_t expected_reads; };

// everything of dg_init / dg_init_files behind the argument checks: contexts objects, index arrays, the upload, the aids
static dg_ctx *init_index(const IndexMeta &m, UpSrc bwt, uint64_t bwt_off, UpSrc sa, uint64_t sa_off, uint64_t sa_first, uint64_t sa_count, UpSrc pac, size_t pac_copy,
                          const dg_params *p, int device, int flags, int *status)
{
    int ndev = 0;
    dg_ctx *c = nullptr;
    auto bail = [&](int code, const char *what, hipError_t e) -> dg_ctx * {
        snprintf(g_init_error, sizeof g_init_error, "%s: %s", what, e == hipSuccess ? "invalid" : hipGetErrorString(e));
        if (c) dg_destroy(c);
        if (status) *status = code;
        return nullptr;
    };
    const double t_start = now_s();
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return bail(DG_ERR_NO_DEVICE, "no HIP device (libdartgpu has no CPU fallback)", e);
    if (device < 0 || device >= ndev) return bail(DG_ERR_NO_DEVICE, "device ordinal out of range", hipSuccess);
    if ((e = hipSetDevice(device)) != hipSuccess) return bail(DG_ERR_HIP, "hipSetDevice", e);
    c = new dg_ctx();
    c->device = device;
    c->shared_caps = new dg_ctx::SharedCaps(); c->owns_shared_caps = true;
    c->shared_ix = new IndexShared(); c->shared_ix->device = device;
    if ((e = make_ctx_objects(c)) != hipSuccess) return bail(DG_ERR_HIP, "stream / event / counter allocation", e);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
    set_params(c, p);
    const double t_ctx = now_s();

    // ---- index arrays: the .bwt blocks at a 64-byte aligned base (+ two blocks of padding so the last, possibly partial, block can be
    //      fetched whole), sampled SA, pac, chromosome keys
    const size_t bwt_bytes = (size_t)m.bwt_words * 4, sa_bytes = (size_t)m.n_sa * 8, pac_bytes = std::max(pac_both_bytes(m.l_pac), (size_t)(m.l_pac / 4 + 1));   // both strands: 2 bits x 2L
    const uint64_t n_blocks = (m.seq_len + 127) / 128;
    if (bwt_bytes > (n_blocks + 1) * 64) return bail(DG_ERR_ARG, "the .bwt data is larger than its header's text length allows", hipSuccess);
    if ((e = hipMalloc(&c->d_bwt, (n_blocks + 2) * 64)) != hipSuccess || (e = hipMemsetAsync(c->d_bwt, 0, (n_blocks + 2) * 64, c->stream)) != hipSuccess) return bail(DG_ERR_HIP, "hipMalloc bwt", e);
    if ((e = hipMalloc(&c->d_sa, sa_bytes + 8)) != hipSuccess || (e = hipMemsetAsync(c->d_sa, 0, sa_bytes + 8, c->stream)) != hipSuccess) return bail(DG_ERR_HIP, "hipMalloc sa", e);
    if ((e = hipMalloc(&c->d_pac, pac_bytes + 4096)) != hipSuccess || (e = hipMemsetAsync(c->d_pac, 0, pac_bytes + 4096, c->stream)) != hipSuccess) return bail(DG_ERR_HIP, "hipMalloc pac", e);
    {
        const int n = m.n_chr;
        std::vector<int64_t> key(2 * n), off(n);
        std::vector<int32_t> chr(2 * n);
        for (int i = 0; i < n; i++) {       // ChrLocMap, bwt_index.cpp:246-250
            off[i] = m.chr_off[i];
            key[i] = m.chr_off[i] + m.chr_len[i] - 1; chr[i] = i;
            key[2 * n - 1 - i] = 2 * m.l_pac - m.chr_off[i] - 1; chr[2 * n - 1 - i] = i;
        }
        if ((e = hipMalloc(&c->d_lockey, 16 * (size_t)n)) != hipSuccess || (e = hipMalloc(&c->d_locchr, 8 * (size_t)n)) != hipSuccess ||
            (e = hipMalloc(&c->d_chroff, 8 * (size_t)n)) != hipSuccess) return bail(DG_ERR_HIP, "hipMalloc chr tables", e);
        if ((e = hipMemcpy(c->d_lockey, key.data(), 16 * (size_t)n, hipMemcpyHostToDevice)) != hipSuccess ||
            (e = hipMemcpy(c->d_locchr, chr.data(), 8 * (size_t)n, hipMemcpyHostToDevice)) != hipSuccess ||
            (e = hipMemcpy(c->d_chroff, off.data(), 8 * (size_t)n, hipMemcpyHostToDevice)) != hipSuccess) return bail(DG_ERR_HIP, "upload chr tables", e);
        if (sa_first) {                    // (from the file: sa[0] = -1 is not stored, bwt.c:185-196)
            const uint64_t minus1 = ~0ull;
            if ((e = hipMemcpyAsync(c->d_sa, &minus1, 8, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return bail(DG_ERR_HIP, "upload sa[0]", e);
        }
    }
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return bail(DG_ERR_HIP, "index array fills", e);
    c->ix.bwt = (const uint4 *)c->d_bwt; c->ix.sa = (const uint64_t *)c->d_sa; c->ix.pac = (const uint8_t *)c->d_pac;
    c->ix.loc_key = (const int64_t *)c->d_lockey; c->ix.loc_chr = (const int32_t *)c->d_locchr; c->ix.chr_off = (const int64_t *)c->d_chroff;
    c->ix.primary = m.primary; for (int i = 0; i < 5; i++) c->ix.L2[i] = m.L2[i]; c->ix.seq_len = m.seq_len;
    c->ix.l_pac = m.l_pac; c->ix.n_chr = m.n_chr; c->ix.sa_intv = m.sa_intv;
    c->ix.ktab = nullptr; c->ix.ktab_k = 0; c->ix.sa_dense = nullptr; c->ix.sa_dense_intv = 0; c->ix.sa_dense_shift = 0;
    c->ix.pac_both = 1;                    // (the second half is filled below, before the first kernel that reads pac can start)
    IndexShared *sh = c->shared_ix;
    sh->ix = c->ix; c->ix_gen = sh->gen.load();
    const double t_alloc = now_s();
    sh->aids_state.store(1);
    sh->aids = std::thread(aids_thread, sh, m.sa_intv, m.n_sa, (flags & DG_INIT_ASYNC_AIDS) != 0, m.expected_reads);   // (sync: allocates the aids while the index bytes travel)

    const size_t chunk = (size_t)32 << 20;
    std::vector<UpChunk> chunks;
    add_chunks(chunks, bwt, bwt_off, (uint8_t *)c->d_bwt, bwt_bytes, chunk, true, n_blocks);
    add_chunks(chunks, sa, sa_off, (uint8_t *)c->d_sa + 8 * sa_first, (size_t)sa_count * 8, chunk, false, 0);
    add_chunks(chunks, pac, 0, (uint8_t *)c->d_pac, pac_copy, chunk, false, 0);
    int n_threads = 6;
    if (const char *v = getenv("DG_INIT_THREADS")) n_threads = std::max(1, std::min(32, atoi(v)));
    n_threads = (int)std::min<size_t>((size_t)n_threads, std::max<size_t>(1, chunks.size()));
    std::string what;
    e = upload_chunks(device, chunks, chunk, n_threads, what);
    const double t_fwd = now_s();
    if (e == hipSuccess && (e = pac_fill_second_half((uint8_t *)c->d_pac, m.l_pac, c->stream)) != hipSuccess) what = "k_pac_both (the second strand of pac)";
    const double t_both = now_s() - t_fwd;
    { std::lock_guard<std::mutex> lk(sh->mu); sh->upload_done = true; sh->upload_ok = e == hipSuccess; }
    sh->cv.notify_all();
    if (e != hipSuccess) return bail(what.find("shorter") != std::string::npos ? DG_ERR_ARG : DG_ERR_HIP, what.c_str(), what.find("shorter") != std::string::npos ? hipSuccess : e);
    {
        std::lock_guard<std::mutex> lk(sh->mu);
        char b[400];
        snprintf(b, sizeof b, "context %.3f s, index arrays (hipMalloc + fill) %.3f s, %s -> HBM + Occ re-layout %.3f s (%.2f GB, %d reader threads), second strand of pac (k_pac_both) %.4f s",
                 t_ctx - t_start, t_alloc - t_ctx, bwt.mem ? "host arrays" : "index files", t_fwd - t_alloc, (bwt_bytes + sa_count * 8 + pac_copy) / 1e9, n_threads, t_both);
        sh->report = std::string(b) + sh->report;
    }
    if (!(flags & DG_INIT_ASYNC_AIDS)) {
        const int rc = dg_index_wait(c);
        if (rc != DG_OK) { char msg[256]; { std::lock_guard<std::mutex> lk(sh->mu); snprintf(msg, sizeof msg, "%s", sh->aids_msg); } snprintf(g_init_error, sizeof g_init_error, "%s", msg); dg_destroy(c); if (status) *status = rc; return nullptr; }
    }
    if (getenv("DG_INIT_TIMING")) fprintf(stderr, "[libdartgpu init] %s%s (total %.3f s)\n", dg_init_report(c), (flags & DG_INIT_ASYNC_AIDS) ? "; aids: building in the background" : "", now_s() - t_start);
    if (status) *status = DG_OK;
    return c;
}

extern "C" int dg_index_wait(dg_ctx *c)
{
    if (!c || !c->shared_ix) return DG_ERR_ARG;
    IndexShared *sh = c->shared_ix;
    {
        std::unique_lock<std::mutex> lk(sh->mu);
        sh->cv.wait(lk, [&]() { const int s = sh->aids_state.load(); return s != 1; });
    }
    refresh_index(c);
    if (sh->aids_state.load() < 0) { std::lock_guard<std::mutex> lk(sh->mu); snprintf(c->err, 512, "look-up aids not built: %s", sh->aids_msg); return DG_ERR_HIP; }
    return DG_OK;
}

extern "C" const char *dg_init_report(const dg_ctx *c)
{
    if (!c || !c->shared_ix) return "";
    IndexShared *sh = c->shared_ix;
    std::lock_guard<std::mutex> lk(sh->mu);
    char q[96];                            // (always the last two fields, whatever the aids thread has appended so far)
    snprintf(q, sizeof q, "; hw_queues_env_found=%s hw_queues_env_set=%d", g_hwq_found, g_hwq_left);
    sh->report_out = sh->report + q;       // (a copy the caller may keep reading while the aids thread appends)
    return sh->report_out.c_str();
}

extern "C" dg_ctx *dg_init(const dg_index_view *v, const dg_params *p, int device, int *status)
{
    if (!v || !p || !v->bwt || !v->sa || !v->pac || v->n_chr <= 0 || v->n_sa == 0) {
        snprintf(g_init_error, sizeof g_init_error, "dg_init arguments: invalid");
        if (status) *status = DG_ERR_ARG;
        return nullptr;
    }
    IndexMeta m;
    m.bwt_words = v->bwt_words; m.primary = v->primary; for (int i = 0; i < 5; i++) m.L2[i] = v->L2[i]; m.seq_len = v->seq_len; m.n_sa = v->n_sa; m.sa_intv = v->sa_intv;
    m.l_pac = v->l_pac; m.n_chr = v->n_chr; m.chr_off = v->chr_off; m.chr_len = v->chr_len; m.expected_reads = 0;
    UpSrc b, s, q;
    b.mem = (const uint8_t *)v->bwt; s.mem = (const uint8_t *)v->sa; q.mem = v->pac;
    return init_index(m, b, 0, s, 0, 0, v->n_sa, q, (size_t)(v->l_pac / 4 + 1), p, device, 0, status);
}

extern "C" dg_ctx *dg_init_files(const dg_index_files *f, const dg_params *p, int device, int flags, int *status)
{
    auto bad = [&](int code, const char *fmt, const char *arg) -> dg_ctx * {
        snprintf(g_init_error, sizeof g_init_error, fmt, arg);
        if (status) *status = code;
        return nullptr;
    };
    if (!f || !p || !f->bwt_path || !f->sa_path || !f->pac_path || f->n_chr <= 0 || !f->chr_off || !f->chr_len || f->l_pac <= 0) return bad(DG_ERR_ARG, "dg_init_files arguments: %s", "invalid");
    struct Fd { int fd = -1; ~Fd() { if (fd >= 0) close(fd); } } fb, fs, fp;
    struct stat st;
    IndexMeta m;
    // .bwt: primary, L2[1..4], then the Occ-interleaved words (bwt_index.cpp:102-121)
    if ((fb.fd = open(f->bwt_path, O_RDONLY)) < 0 || fstat(fb.fd, &st) != 0 || st.st_size < 40) return bad(DG_ERR_ARG, "cannot read %s", f->bwt_path);
    uint64_t hdr[7];
    if (pread(fb.fd, hdr, 40, 0) != 40) return bad(DG_ERR_ARG, "cannot read %s", f->bwt_path);
    m.primary = hdr[0]; m.L2[0] = 0; for (int i = 1; i < 5; i++) m.L2[i] = hdr[i]; m.seq_len = m.L2[4];
    m.bwt_words = ((uint64_t)st.st_size - 40) / 4;
    // .sa: primary, L2[1..4], sa_intv, seq_len, then sa[1 .. n_sa) (bwt_index.cpp:15-35)
    if ((fs.fd = open(f->sa_path, O_RDONLY)) < 0 || fstat(fs.fd, &st) != 0 || st.st_size < 56) return bad(DG_ERR_ARG, "cannot read %s", f->sa_path);
    if (pread(fs.fd, hdr, 56, 0) != 56) return bad(DG_ERR_ARG, "cannot read %s", f->sa_path);
    m.sa_intv = (int)hdr[5];
    if (m.sa_intv <= 0 || m.seq_len == 0) return bad(DG_ERR_ARG, "%s: bad header", f->sa_path);
    m.n_sa = (m.seq_len + (uint64_t)m.sa_intv) / (uint64_t)m.sa_intv;
    const uint64_t sa_count = std::min<uint64_t>(m.n_sa - 1, ((uint64_t)st.st_size - 56) / 8);
    if ((fp.fd = open(f->pac_path, O_RDONLY)) < 0 || fstat(fp.fd, &st) != 0) return bad(DG_ERR_ARG, "cannot read %s", f->pac_path);
    const size_t pac_copy = std::min<size_t>((size_t)st.st_size, (size_t)(f->l_pac / 4 + 1));
    m.l_pac = f->l_pac; m.n_chr = f->n_chr; m.chr_off = f->chr_off; m.chr_len = f->chr_len; m.expected_reads = f->expected_reads;
    UpSrc b, s, q;
    b.fd = fb.fd; s.fd = fs.fd; q.fd = fp.fd;
    return init_index(m, b, 40, s, 56, 1, sa_count, q, pac_copy, p, device, flags, status);
}

// A second context on the same device that shares the parent's index (no copy): its own streams, batch buffers
// and counters, so that two batches can be in flight at once (one host thread per context).  The parent must
// outlive its clones.  (The hardware queues the contexts' streams need: dg_default_hw_queues, at the top of this file.)
extern "C" dg_ctx *dg_clone(dg_ctx *parent, int *status)
{
    if (status) *status = DG_ERR_ARG;
    if (!parent) return nullptr;
    hipError_t e;
    if ((e = hipSetDevice(parent->device)) != hipSuccess) { if (status) *status = DG_ERR_HIP; return nullptr; }
    dg_ctx *c = new dg_ctx();
    c->device = parent->device; c->owns_index = false; c->n_cu = parent->n_cu;
    c->shared_ix = parent->shared_ix;
    c->ix = parent->ix; c->ix_gen = parent->ix_gen; c->pr = parent->pr;
    refresh_index(c);
    c->shared_caps = parent->shared_caps;
    if ((e = make_ctx_objects(c)) != hipSuccess) {
        snprintf(g_init_error, sizeof g_init_error, "dg_clone: %s", hipGetErrorString(e)); dg_destroy(c); if (status) *status = DG_ERR_HIP; return nullptr;
    }
    // more streams than hardware queues: which contexts share one -- and run their kernels one behind the other -- then changes from process to
    // process.  Said once per process, when it first happens.
    const int live = g_live_ctx[c->device & 63].load();
    if (live + 2 > g_hwq_left && !g_hwq_warned.exchange(true))
        fprintf(stderr, "[libdartgpu] %d contexts on device %d + the copy stream + the caller's stream are more than the %d hardware queues of this process "
                        "(GPU_MAX_HW_QUEUES was %s when the library loaded and %d when its constructor returned): contexts will share queues and wait for each other\n",
                live, c->device, g_hwq_left, g_hwq_found, g_hwq_left);
    if (status) *status = DG_OK;
    return c;
}

// ------------------------------------------------------------------------------------------
// batch input: ASCII reads (as the reference's ReadItem_t::seq) or packed reads (2 bit/base + a list of the non-ACGT positions)
// ------------------------------------------------------------------------------------------
static int enqueue_upload(dg_ctx *c, int n_reads, const uint32_t *seq_off, const uint16_t *rlen, const char *seq)
{
    if (!c || n_reads < 0 || (n_reads > 0 && (!seq_off || !rlen || !seq))) return DG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    size_t bytes = 0; int mx = 0;
    for (int i = 0; i < n_reads; i++) {
        const size_t end = (size_t)seq_off[i] + rlen[i];
        bytes = end > bytes ? end : bytes;
        mx = rlen[i] > mx ? rlen[i] : mx;
    }
    if (mx > DG_MAX_RLEN) { snprintf(c->err, 512, "a read is longer than DG_MAX_RLEN (%d)", DG_MAX_RLEN); return DG_ERR_ARG; }
    c->n_reads = n_reads; c->max_rlen = mx; c->seq_bytes = bytes; c->enc_ready = false; c->enqueued = false; c->batch_done = false; c->sj.batch_counted = false; c->gc.batch_counted = false; c->tx.batch_counted = false; c->sam.valid = false; c->bam.valid = false; c->bam.rec_valid = false; c->bam.rec_stored = false; c->fq.valid = false;
    c->no_batch = false; c->inf.valid = false;
    HIPCHK(c->seq.ensure(bytes + 64));     /* the kernels read up to 24 bytes at a read position in one go */
    HIPCHK(c->seq_off.ensure((size_t)n_reads + 1)); HIPCHK(c->rlen.ensure((size_t)n_reads + 1));
    if (n_reads) {
        HIPCHK(hipMemcpyAsync(c->seq.p, seq, bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->seq_off.p, seq_off, (size_t)n_reads * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->rlen.p, rlen, (size_t)n_reads * 2, hipMemcpyHostToDevice, c->stream));
    }
    return DG_OK;
}

extern "C" int dg_batch_upload(dg_ctx *c, int n_reads, const uint32_t *seq_off, const uint16_t *rlen, const char *seq)
{
    const int rc = enqueue_upload(c, n_reads, seq_off, rlen, seq);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return DG_OK;
}

// packed reads -> the ASCII buffer the report stage reads (A/C/G/T, then 'N' at the listed positions) and the 2-bit + mask
// words the seeding stage reads (k_encode's format).  One thread = 16 bases = one input word.
__global__ void __launch_bounds__(256)
k_unpack(const uint32_t *__restrict__ words, uint32_t n_words, int W2, double inv_w2, int rlen_all, const uint16_t *rlen_in, unsigned char *__restrict__ seq,
         uint32_t *__restrict__ seq_off, uint16_t *rlen_out, uint32_t *__restrict__ enc, unsigned int *bad)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_words) return;
    if (t == 0) *bad = 0u;                                              // (k_unpack_n, the next launch, raises it)
    uint32_t r = (uint32_t)((double)t * inv_w2);                        // t / W2 without an integer division: the product is within one of it
    if (r * (uint32_t)W2 > t) r--; else if ((r + 1u) * (uint32_t)W2 <= t) r++;
    const int ww = (int)(t - r * (uint32_t)W2);
    const int len = rlen_in ? rlen_in[r] : rlen_all, left = len - 16 * ww;
    const uint32_t w = words[t];
    // (no ASCII copy of the batch: the seeding stage and the fused pair kernel read the words; k_prep rebuilds the characters of the
    //  units that take the general path -- a twentieth of a DNA batch)
    const uint32_t past = left >= 16 ? 0u : (left <= 0 ? 0xFFFFFFFFu : 0xFFFFFFFFu >> (2 * left));          // mask 0b11 past the end, as k_encode
    enc[(size_t)r * 2 * W2 + ww] = w & ~past;
    enc[(size_t)r * 2 * W2 + W2 + ww] = past;
    if (ww == 0) { seq_off[r] = r * 16u * (uint32_t)W2; if (!rlen_in) rlen_out[r] = (uint16_t)len; }      // (given lengths are already in place)
}
__global__ void __launch_bounds__(256)
k_unpack_n(const uint32_t *__restrict__ nlist, uint32_t n_n, int W2, uint32_t n_bases, unsigned char *__restrict__ seq, uint32_t *__restrict__ enc, unsigned int *bad)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_n) return;
    const uint32_t flat = nlist[i], per = 16u * (uint32_t)W2, r = flat / per, pos = flat - r * per;
    if (flat >= n_bases) { atomicMax(bad, 1u); return; }       // a list entry outside the batch (a buggy packer) must not write outside it: dg_batch_run reports DG_ERR_ARG
    const uint32_t bit = 3u << (30 - 2 * (pos & 15u));
    atomicAnd(&enc[(size_t)r * 2 * W2 + (pos >> 4)], ~bit);
    atomicOr(&enc[(size_t)r * 2 * W2 + W2 + (pos >> 4)], bit);
}

static int enqueue_upload_packed(dg_ctx *c, int n_reads, int rlen_all, const uint16_t *rlen, int words_per_read, const uint32_t *words, const uint32_t *nlist, size_t n_n)
{
    if (!c || n_reads < 0 || words_per_read < 1 || (n_reads > 0 && !words) || (n_n > 0 && !nlist)) return DG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    const int W2 = words_per_read;
    int mx = rlen_all;
    if (rlen) { mx = 0; for (int i = 0; i < n_reads; i++) mx = rlen[i] > mx ? rlen[i] : mx; }
    if (mx > DG_MAX_RLEN || mx > 16 * W2 || (size_t)n_reads * 16 * W2 > 0xFFFFFFF0ull) { snprintf(c->err, 512, "packed batch: read length %d does not fit %d words (or exceeds DG_MAX_RLEN / 2^32 bases)", mx, W2); return DG_ERR_ARG; }
    if (n_reads && (mx + 15) / 16 != W2) { snprintf(c->err, 512, "packed batch: words_per_read must be ceil(longest read / 16) = %d", (mx + 15) / 16); return DG_ERR_ARG; }
    const size_t nw = (size_t)n_reads * W2, bytes = nw * 16;
    c->n_reads = n_reads; c->max_rlen = mx; c->seq_bytes = bytes; c->enqueued = false; c->batch_done = false; c->sj.batch_counted = false; c->gc.batch_counted = false; c->tx.batch_counted = false; c->sam.valid = false; c->bam.valid = false; c->bam.rec_valid = false; c->bam.rec_stored = false; c->fq.valid = false;
    c->no_batch = false; c->inf.valid = false;
    HIPCHK(c->seq.ensure(bytes + 64)); HIPCHK(c->seq_off.ensure((size_t)n_reads + 1)); HIPCHK(c->rlen.ensure((size_t)n_reads + 1));
    HIPCHK(c->enc.ensure(2 * nw + 16)); HIPCHK(c->packed_in.ensure(nw + 1)); HIPCHK(c->nlist_in.ensure(n_n + 1));
    c->enc_ready = true;
    if (n_reads == 0) return DG_OK;
    HIPCHK(hipMemcpyAsync(c->packed_in.p, words, nw * 4, hipMemcpyHostToDevice, c->stream));
    if (rlen) HIPCHK(hipMemcpyAsync(c->rlen.p, rlen, (size_t)n_reads * 2, hipMemcpyHostToDevice, c->stream));
    if (n_n) HIPCHK(hipMemcpyAsync(c->nlist_in.p, nlist, n_n * 4, hipMemcpyHostToDevice, c->stream));
    k_unpack<<<(unsigned)((nw + 255) / 256), 256, 0, c->stream>>>(c->packed_in.p, (uint32_t)nw, W2, 1.0 / (double)W2, rlen_all, rlen ? c->rlen.p : nullptr, c->seq.p, c->seq_off.p, c->rlen.p, c->enc.p, c->d_input_bad);
    if (n_n) {
        k_unpack_n<<<(unsigned)((n_n + 255) / 256), 256, 0, c->stream>>>(c->nlist_in.p, (uint32_t)n_n, W2, (uint32_t)(nw * 16), c->seq.p, c->enc.p, c->d_input_bad);
        HIPCHK(hipMemcpyAsync(&c->h_tail->input_bad, c->d_input_bad, 4, hipMemcpyDeviceToHost, c->stream));
    } else c->h_tail->input_bad = 0;
    HIPCHK(hipGetLastError());
    return DG_OK;
}

extern "C" int dg_batch_upload_packed(dg_ctx *c, int n_reads, int rlen_all, const uint16_t *rlen, int words_per_read, const uint32_t *words, const uint32_t *nlist, size_t n_n)
{
    const int rc = enqueue_upload_packed(c, n_reads, rlen_all, rlen, words_per_read, words, nlist, n_n);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return DG_OK;
}

// ------------------------------------------------------------------------------------------
// batch input as FASTQ text (dg_fastq.h): the file bytes go up once, six kernels cut them into the batch -- bases, names, stored qualities -- in HBM
// ------------------------------------------------------------------------------------------
extern "C" int dg_fastq_tile(void) { return FQ_TILE; }

// The parser behind its input: the texts lie in c->fq.text, text 1 at 0 and text 2 at off2.  fq_reserve sizes every buffer from the arguments (nothing is asked
// of the device before the one wait), fq_enqueue launches the kernels, fq_finish waits for the sizes block and says what it holds.
struct FqPlan { size_t n[2], off2, line_cap[2], tile_stride, reads_bound, len_tiles, max_reads, text_bytes; bool two; };

static int fq_reserve(dg_ctx *c, FqPlan &p)
{
    HIPCHK(c->fq.ready());
    if (c->tr.any()) HIPCHK(c->tr.ready());
    // a record has at least one byte per existing line, so a text of n bytes holds at most n + 1 line starts; the three outputs together are never larger
    // than the texts
    const size_t max_reads = p.max_reads, n1 = p.n[0], n2 = p.n[1];
    const size_t rec_cap[2] = { p.two ? (max_reads + 1) / 2 : max_reads, p.two ? max_reads / 2 : 0 };
    size_t tiles[2];
    for (int f = 0; f < 2; f++) { p.line_cap[f] = std::min(4 * rec_cap[f] + 1, p.n[f] + 1); tiles[f] = (p.n[f] + FQ_TILE - 1) / FQ_TILE; }
    p.off2 = (n1 + 16 + 255) & ~(size_t)255; p.text_bytes = n1 + n2;
    p.tile_stride = std::max(tiles[0], tiles[1]);
    p.reads_bound = std::min(max_reads, (n1 + 4) / 4 + (n2 + 4) / 4);          // (records <= ceil(lines / 4), lines <= bytes + 1)
    p.len_tiles = std::max<size_t>(1, (p.reads_bound + FQ_THREADS - 1) / FQ_THREADS);
    const size_t reads_bound = p.reads_bound, text_bytes = p.text_bytes;
    HIPCHK(c->fq.text.ensure(p.off2 + n2 + 32)); HIPCHK(c->fq.lines.ensure(p.line_cap[0] + p.line_cap[1] + 2)); HIPCHK(c->fq.tile_cnt.ensure(2 * p.tile_stride + 1));
    HIPCHK(c->fq.name_at.ensure(reads_bound + 1)); HIPCHK(c->fq.name_len.ensure(reads_bound + 1)); HIPCHK(c->fq.loc.ensure(4 * (reads_bound + 1))); HIPCHK(c->fq.tile_sum.ensure(4 * p.len_tiles));      // (the fourth row: the trimmed path's keep flags)
    if (c->tr.any()) HIPCHK(c->tr.win.ensure(reads_bound + 1));
    HIPCHK(c->fq.hdr_off.ensure(reads_bound + 1)); HIPCHK(c->fq.qual_off.ensure(reads_bound + 1)); HIPCHK(c->fq.qual.ensure(text_bytes + 1));
    HIPCHK(c->fq.hdr.ensure(text_bytes + 1 + (c->tr.umi_on ? 22 * (reads_bound + 1) : 0)));      // (dg_set_umi: a name gains the separator and at most 21 letters)
    HIPCHK(c->seq.ensure(text_bytes + 64)); HIPCHK(c->seq_off.ensure(reads_bound + 1)); HIPCHK(c->rlen.ensure(reads_bound + 1));
    return DG_OK;
}

// the context trims (dg_set_trim): behind the line kernels the windows are cut, and the length, sum and writing kernels are the ones of dg_trim.h
static int fq_enqueue_trimmed(dg_ctx *c, const FqPlan &p, const FqText &x, int rc_odd_reads, bool write)
{
    const uint32_t stride = (uint32_t)(p.reads_bound + 1);
    const TrimPar par = c->tr.effective();
    HIPCHK(hipMemsetAsync(c->tr.info.d, 0, sizeof(TrimInfo), c->stream));
    HIPCHK(hipEventRecord(c->tr.ev[0], c->stream));
    if (p.reads_bound) k_trim_cut<<<(unsigned)p.reads_bound, 64, 0, c->stream>>>(x, c->fq.info.d, par, c->tr.win.p);
    k_trim_len<<<(unsigned)p.len_tiles, FQ_THREADS, 0, c->stream>>>(x, c->fq.info.d, par, c->tr.win.p, c->tr.info.d, c->fq.name_at.p, c->fq.name_len.p, c->fq.loc.p, stride, c->fq.tile_sum.p,
                                                                     (uint32_t)p.len_tiles);
    k_trim_top3<<<1, FQ_THREADS, 0, c->stream>>>(c->fq.tile_sum.p, (uint32_t)p.len_tiles, c->fq.info.d, c->tr.info.d);
    if (p.reads_bound && write)
        k_trim_write<<<(unsigned)p.reads_bound, 64, 0, c->stream>>>(x, c->fq.info.d, c->tr.info.d, rc_odd_reads ? 1 : 0, c->tr.win.p, c->fq.name_at.p, c->fq.name_len.p, c->fq.loc.p, stride,
                                                                     c->fq.tile_sum.p, (uint32_t)p.len_tiles, c->rlen.p, c->seq_off.p, c->seq.p, c->fq.hdr_off.p, c->fq.hdr.p, c->fq.qual_off.p,
                                                                     c->fq.qual.p);
    if (p.reads_bound && write && par.umi_on)
        k_trim_umi_name<<<(unsigned)p.reads_bound, 64, 0, c->stream>>>(x, c->fq.info.d, TrimUmi{par.umi_on, par.umi_flags, {par.umi_len[0], par.umi_len[1]}, par.umi_sep}, c->tr.win.p, c->fq.name_len.p,
                                                                        c->fq.loc.p, stride, c->fq.tile_sum.p, (uint32_t)p.len_tiles, c->fq.hdr.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->tr.ev[1], c->stream));
    HIPCHK(hipEventRecord(c->fq.ev[1], c->stream));
    HIPCHK(c->fq.info.fetch(c->stream));
    HIPCHK(c->tr.info.fetch(c->stream));
    c->tr.enqueued = true;
    return DG_OK;
}

// whole: the texts are pieces of files (whole records only; the tails and the count of unlike records are taken too); write: the batch is written
static int fq_enqueue(dg_ctx *c, const FqPlan &p, int rc_odd_reads, bool whole, bool pieces, bool write)
{
    FqText x;
    x.t[0] = c->fq.text.p; x.t[1] = c->fq.text.p + p.off2; x.n[0] = (uint32_t)p.n[0]; x.n[1] = (uint32_t)p.n[1];
    x.line_start[0] = c->fq.lines.p; x.line_start[1] = c->fq.lines.p + p.line_cap[0] + 1; x.line_cap[0] = (uint32_t)p.line_cap[0]; x.line_cap[1] = (uint32_t)p.line_cap[1];
    x.two = p.two ? 1 : 0;
    const uint32_t stride = (uint32_t)(p.reads_bound + 1);
    const dim3 text_grid((unsigned)std::max<size_t>(1, p.tile_stride), p.two ? 2u : 1u);
    k_fq_count<<<text_grid, FQ_THREADS, 0, c->stream>>>(x, c->fq.tile_cnt.p, (uint32_t)p.tile_stride);
    k_fq_top<<<1, FQ_THREADS, 0, c->stream>>>(x, c->fq.tile_cnt.p, (uint32_t)p.tile_stride, (uint32_t)p.max_reads, c->fq.info.d, whole ? 1 : 0);
    k_fq_lines<<<text_grid, FQ_THREADS, 0, c->stream>>>(x, c->fq.tile_cnt.p, (uint32_t)p.tile_stride, c->fq.info.d);
    if (whole) k_fq_tail<<<dim3(64, p.two ? 2u : 1u), FQ_THREADS, 0, c->stream>>>(x, c->fq.info.d, c->fq.tail.p, (uint32_t)c->fq.tail_off2);
    if (pieces && p.reads_bound) k_fq_unlike<<<(unsigned)p.reads_bound, 64, 0, c->stream>>>(x, c->fq.info.d);
    if (c->tr.any()) return fq_enqueue_trimmed(c, p, x, rc_odd_reads, write);
    k_fq_len<<<(unsigned)p.len_tiles, FQ_THREADS, 0, c->stream>>>(x, c->fq.info.d, c->rlen.p, c->fq.name_at.p, c->fq.name_len.p, c->fq.loc.p, stride, c->fq.tile_sum.p, (uint32_t)p.len_tiles);
    k_fq_top3<<<1, FQ_THREADS, 0, c->stream>>>(c->fq.tile_sum.p, (uint32_t)p.len_tiles, c->fq.info.d);
    if (p.reads_bound && write)
        k_fq_write<<<(unsigned)p.reads_bound, 64, 0, c->stream>>>(x, c->fq.info.d, rc_odd_reads ? 1 : 0, c->rlen.p, c->fq.name_at.p, c->fq.name_len.p, c->fq.loc.p, stride, c->fq.tile_sum.p,
                                                                   (uint32_t)p.len_tiles, c->seq_off.p, c->seq.p, c->fq.hdr_off.p, c->fq.hdr.p, c->fq.qual_off.p, c->fq.qual.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->fq.ev[1], c->stream));
    HIPCHK(c->fq.info.fetch(c->stream));
    return DG_OK;
}

// behind the wait: the sizes block's verdict; keep: the context holds the batch from here on
static int fq_finish(dg_ctx *c, const char *fn, int max_reads, int *n_reads_out, bool keep)
{
    c->fq.ms = c->fq.ev.ms(0, 1);
    const FqInfo &fi = *c->fq.info.h;
    const bool trimmed = c->tr.enqueued;
    c->tr.enqueued = false;
    if (n_reads_out) *n_reads_out = (int)std::min<uint32_t>(fi.n_reads, 0x7FFFFFFFu);
    switch (fi.status) {
    case FQ_OK: break;
    case FQ_E_COUNT:
        snprintf(c->err, 512, "%s: text1 holds %u records and text2 %u: they must be equal, or text1 one more", fn, (fi.n_lines[0] + 3) / 4, (fi.n_lines[1] + 3) / 4);
        return DG_ERR_ARG;
    case FQ_E_CAPACITY:
        snprintf(c->err, 512, "%s: the texts hold %u reads, max_reads is %d", fn, fi.n_reads, max_reads);
        return DG_ERR_CAPACITY;
    case FQ_E_EMPTY:
        snprintf(c->err, 512, "%s: read %u is a record without bases", fn, fi.bad_read);
        return DG_ERR_ARG;
    case FQ_E_LONG:
        snprintf(c->err, 512, "%s: read %u is longer than DG_MAX_RLEN (%d)", fn, fi.bad_read, DG_MAX_RLEN);
        return DG_ERR_ARG;
    default:
        snprintf(c->err, 512, "%s: the bases, names or qualities of the batch exceed 32-bit offsets", fn);
        return DG_ERR_ARG;
    }
    uint32_t n_reads = fi.n_reads;
    if (trimmed) {                                               // the batch is the kept reads
        const TrimInfo &ti = *c->tr.info.h;
        memcpy(c->tr.stats, ti.stats, sizeof c->tr.stats); c->tr.ms = c->tr.ev.ms(0, 1);
        n_reads = ti.n_kept;
        if (n_reads_out) *n_reads_out = (int)n_reads;
    }
    if (!keep) return DG_OK;
    c->n_reads = (int)n_reads; c->max_rlen = (int)fi.max_rlen; c->seq_bytes = (size_t)fi.total[0];
    c->fq.hdr_bytes = (size_t)fi.total[1]; c->fq.qual_bytes = (size_t)fi.total[2]; c->fq.valid = true;
    return DG_OK;
}

// whatever happens in an upload of FASTQ text, the context holds no batch until the call has succeeded
static void fq_forget_batch(dg_ctx *c)
{
    c->n_reads = 0; c->max_rlen = 0; c->seq_bytes = 0; c->enc_ready = false; c->enqueued = false; c->batch_done = false; c->sj.batch_counted = false; c->gc.batch_counted = false; c->tx.batch_counted = false; c->sam.valid = false; c->bam.valid = false; c->bam.rec_valid = false; c->bam.rec_stored = false; c->fq.valid = false;
    c->fq.hdr_bytes = c->fq.qual_bytes = 0; c->fq.ms = 0.f;
    memset(c->tr.stats, 0, sizeof c->tr.stats); c->tr.ms = 0.f; c->tr.enqueued = false;
    c->no_batch = false; c->inf.valid = false; c->fq.tail_valid = false; c->fq.tail_n[0] = c->fq.tail_n[1] = 0;
}

extern "C" int dg_batch_upload_fastq(dg_ctx *c, const dg_fastq_text *in, int *n_reads_out)
{
    if (!c) return DG_ERR_ARG;
    if (n_reads_out) *n_reads_out = 0;
    fq_forget_batch(c);
    if (!in) { snprintf(c->err, 512, "dg_batch_upload_fastq: the input is NULL"); return DG_ERR_ARG; }
    const size_t n1 = in->text1 ? in->n1 : 0, n2 = in->text2 ? in->n2 : 0;
    const bool two = in->text2 != nullptr && in->n2 > 0;
    if ((in->n1 && !in->text1) || in->max_reads < 0) { snprintf(c->err, 512, "dg_batch_upload_fastq: text1 is NULL or max_reads is negative"); return DG_ERR_ARG; }
    if (n1 >= 0xFFFFFF00ull || n2 >= 0xFFFFFF00ull) { snprintf(c->err, 512, "dg_batch_upload_fastq: a text must be smaller than 2^32 - 256 bytes"); return DG_ERR_ARG; }
    if (n1 == 0 && !two) { c->fq.valid = true; return DG_OK; }       // no text: no reads
    HIPCHK(hipSetDevice(c->device));
    FqPlan p;
    p.n[0] = n1; p.n[1] = n2; p.two = two; p.max_reads = (size_t)in->max_reads;
    { const int rc = fq_reserve(c, p); if (rc) return rc; }
    if (n1) HIPCHK(hipMemcpyAsync(c->fq.text.p, in->text1, n1, hipMemcpyHostToDevice, c->stream));
    if (n2) HIPCHK(hipMemcpyAsync(c->fq.text.p + p.off2, in->text2, n2, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->fq.ev[0], c->stream));
    { const int rc = fq_enqueue(c, p, in->rc_odd_reads, false, false, true); if (rc) return rc; }
    HIPCHK(wait_stream(c));                                       // the one wait: for the sizes block
    return fq_finish(c, "dg_batch_upload_fastq", in->max_reads, n_reads_out, true);
}

// ------------------------------------------------------------------------------------------
// BGZF inflated on the device (dg_inflate.h): whole blocks in host memory -> their bytes in HBM; and in front of the FASTQ parser
// ------------------------------------------------------------------------------------------
// the compressed bytes of up to two inputs (the second at in_off2 of inf.in) and the table go up; the kernel writes at d_out + the members' out_off
static int inf_enqueue_copies(dg_ctx *c, const std::vector<InfBlock> &tab, const void *src1, size_t n1, const void *src2, size_t n2, size_t in_off2)
{
    HIPCHK(c->inf.in.ensure(std::max(n1, in_off2 + n2) + 8)); HIPCHK(c->inf.tab.ensure(tab.size() + 1)); HIPCHK(c->inf.status.ensure(tab.size() + 1));
    if (n1) HIPCHK(hipMemcpyAsync(c->inf.in.p, src1, n1, hipMemcpyHostToDevice, c->stream));
    if (n2) HIPCHK(hipMemcpyAsync(c->inf.in.p + in_off2, src2, n2, hipMemcpyHostToDevice, c->stream));
    if (!tab.empty()) HIPCHK(hipMemcpyAsync(c->inf.tab.p, tab.data(), tab.size() * sizeof(InfBlock), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(c->inf.verdict.d, 0xff, 8, c->stream));
    return DG_OK;
}
static int inf_enqueue_kernel(dg_ctx *c, size_t n_blocks, unsigned char *d_out)
{
    if (n_blocks) k_bgzf_inflate<<<(unsigned)((n_blocks + INF_WAVES - 1) / INF_WAVES), 64 * INF_WAVES, 0, c->stream>>>(c->inf.in.p, c->inf.tab.p, (uint32_t)n_blocks, d_out, c->inf.status.p, c->inf.verdict.d);
    HIPCHK(hipGetLastError());
    HIPCHK(c->inf.verdict.fetch(c->stream));
    return DG_OK;
}

extern "C" int dg_inflate_granules(int out[2])
{
    if (!out) return DG_ERR_ARG;
    out[0] = INF_WAVES; out[1] = (int)INF_ROUND;
    return DG_OK;
}

extern "C" int dg_bgzf_inflate(dg_ctx *c, const void *host_bytes, size_t n, size_t *n_out, size_t *n_blocks, float *device_ms)
{
    if (!c) return DG_ERR_ARG;
    if (n_out) *n_out = 0;
    if (n_blocks) *n_blocks = 0;
    if (device_ms) *device_ms = 0.f;
    c->inf.valid = false; c->inf.bytes = 0;
    if (n == 0) { c->inf.valid = true; return DG_OK; }
    if (!host_bytes) { snprintf(c->err, 512, "dg_bgzf_inflate: the input is NULL"); return DG_ERR_ARG; }
    std::vector<InfBlock> tab;
    size_t total = 0, bad = 0;
    if (const char *why = inf_walk_members((const unsigned char *)host_bytes, n, 0, 0, tab, &total, &bad)) { snprintf(c->err, 512, "dg_bgzf_inflate: block %zu: %s", bad, why); return DG_ERR_ARG; }
    if (tab.size() > 0x7fffffffull) { snprintf(c->err, 512, "dg_bgzf_inflate: %zu blocks are more than one call takes", tab.size()); return DG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->inf.ready());
    HIPCHK(c->inf.out.ensure(total + 32));
    { const int rc = inf_enqueue_copies(c, tab, host_bytes, n, nullptr, 0, 0); if (rc) return rc; }
    HIPCHK(hipEventRecord(c->inf.ev[0], c->stream));
    { const int rc = inf_enqueue_kernel(c, tab.size(), c->inf.out.p); if (rc) return rc; }
    HIPCHK(hipEventRecord(c->inf.ev[1], c->stream));
    HIPCHK(wait_stream(c));
    const float ms = c->inf.ev.ms(0, 1);
    if (device_ms) *device_ms = ms;
    if (n_blocks) *n_blocks = tab.size();
    const unsigned long long v = *c->inf.verdict.h;
    if (v != ~0ull) { snprintf(c->err, 512, "dg_bgzf_inflate: block %llu: %s", v >> 8, inf_rule((uint32_t)(v & 0xffu))); return DG_ERR_ARG; }
    c->inf.valid = true; c->inf.bytes = total;
    if (n_out) *n_out = total;
    return DG_OK;
}

extern "C" int dg_inflate_download(dg_ctx *c, void *out, size_t cap)
{
    if (!c) return DG_ERR_ARG;
    if (!c->inf.valid) { snprintf(c->err, 512, "dg_inflate_download: no inflated bytes (dg_bgzf_inflate first)"); return DG_ERR_ARG; }
    if (cap < c->inf.bytes) { snprintf(c->err, 512, "dg_inflate_download: output capacity too small: %zu bytes of %zu", cap, c->inf.bytes); return DG_ERR_CAPACITY; }
    if (c->inf.bytes == 0) return DG_OK;
    if (!out) return DG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(out, c->inf.out.p, c->inf.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));
    return DG_OK;
}

extern "C" int dg_inflate_device(dg_ctx *c, void **ptr, size_t *n_out)
{
    if (!c || !ptr || !n_out) return DG_ERR_ARG;
    if (!c->inf.valid) { snprintf(c->err, 512, "dg_inflate_device: no inflated bytes (dg_bgzf_inflate first)"); return DG_ERR_ARG; }
    *ptr = c->inf.bytes ? c->inf.out.p : nullptr; *n_out = c->inf.bytes;
    return DG_OK;
}

extern "C" int dg_batch_upload_fastq_bgzf(dg_ctx *c, const dg_fastq_bgzf *in, uint32_t flags, int *n_reads_out, size_t tail[2], uint64_t *n_unlike)
{
    static const char *fn = "dg_batch_upload_fastq_bgzf";
    if (!c) return DG_ERR_ARG;
    if (n_reads_out) *n_reads_out = 0;
    if (tail) tail[0] = tail[1] = 0;
    if (n_unlike) *n_unlike = 0;
    fq_forget_batch(c);
    if (!in) { snprintf(c->err, 512, "%s: the input is NULL", fn); return DG_ERR_ARG; }
    if (flags & ~DG_FQ_CHECK_ONLY) { snprintf(c->err, 512, "%s: unknown flag bits 0x%x", fn, flags & ~DG_FQ_CHECK_ONLY); return DG_ERR_ARG; }
    const bool check_only = (flags & DG_FQ_CHECK_ONLY) != 0, two = in->blocks2 != nullptr || in->head2 != nullptr, last = in->last != 0;
    if ((in->n_head1 && !in->head1) || (in->n_blocks1 && !in->blocks1) || (in->n_head2 && !in->head2) || (in->n_blocks2 && !in->blocks2) || in->max_reads < 0) {
        snprintf(c->err, 512, "%s: a length without its pointer, or max_reads is negative", fn); return DG_ERR_ARG;
    }
    // the members of both inputs, before anything is enqueued: text f = head f ++ its blocks' bytes, in fq.text at 0 / off2
    const size_t nh[2] = { in->head1 ? in->n_head1 : 0, in->head2 ? in->n_head2 : 0 }, nb[2] = { in->blocks1 ? in->n_blocks1 : 0, two && in->blocks2 ? in->n_blocks2 : 0 };
    const unsigned char *src[2] = { (const unsigned char *)in->blocks1, (const unsigned char *)in->blocks2 };
    const size_t in_off2 = (nb[0] + 255) & ~(size_t)255;
    std::vector<InfBlock> tab;
    size_t n_inf[2] = {0, 0}, first2 = 0;
    for (int f = 0; f < (two ? 2 : 1); f++) {
        size_t bad = 0;
        if (f) first2 = tab.size();
        if (const char *why = inf_walk_members(src[f], nb[f], f ? in_off2 : 0, nh[f], tab, &n_inf[f], &bad)) { snprintf(c->err, 512, "%s: text %d block %zu: %s", fn, f + 1, bad, why); return DG_ERR_ARG; }
        if (nh[f] + n_inf[f] >= 0xFFFFFF00ull) { snprintf(c->err, 512, "%s: a text must be smaller than 2^32 - 256 bytes", fn); return DG_ERR_ARG; }
    }
    if (!two) first2 = tab.size();
    if (tab.size() > 0x7fffffffull) { snprintf(c->err, 512, "%s: %zu blocks are more than one call takes", fn, tab.size()); return DG_ERR_ARG; }
    FqPlan p;
    p.n[0] = nh[0] + n_inf[0]; p.n[1] = nh[1] + n_inf[1]; p.two = two; p.max_reads = (size_t)in->max_reads;
    if (p.n[0] == 0 && p.n[1] == 0) { c->fq.valid = !check_only; c->no_batch = check_only; c->fq.tail_valid = true; return DG_OK; }       // no text: no reads, no tails
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->inf.ready());
    { const int rc = fq_reserve(c, p); if (rc) return rc; }
    for (size_t k = first2; k < tab.size(); k++) tab[k].out_off += p.off2;
    c->fq.tail_off2 = (p.n[0] + 255) & ~(size_t)255;
    HIPCHK(c->fq.tail.ensure(c->fq.tail_off2 + p.n[1] + 16));
    { const int rc = inf_enqueue_copies(c, tab, src[0], nb[0], src[1], nb[1], in_off2); if (rc) return rc; }
    if (nh[0]) HIPCHK(hipMemcpyAsync(c->fq.text.p, in->head1, nh[0], hipMemcpyHostToDevice, c->stream));
    if (nh[1]) HIPCHK(hipMemcpyAsync(c->fq.text.p + p.off2, in->head2, nh[1], hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->fq.ev[0], c->stream));
    { const int rc = inf_enqueue_kernel(c, tab.size(), c->fq.text.p); if (rc) return rc; }
    { const int rc = fq_enqueue(c, p, in->rc_odd_reads, !last, true, !check_only); if (rc) return rc; }
    HIPCHK(wait_stream(c));                                       // the one wait: for the first failing block and the sizes block
    const unsigned long long v = *c->inf.verdict.h;
    if (v != ~0ull) {                                             // (the parser ran over bytes that mean nothing: its verdict is not looked at)
        const size_t k = (size_t)(v >> 8);
        snprintf(c->err, 512, "%s: text %d block %zu: %s", fn, k >= first2 ? 2 : 1, k >= first2 ? k - first2 : k, inf_rule((uint32_t)(v & 0xffu)));
        return DG_ERR_ARG;
    }
    const FqInfo &fi = *c->fq.info.h;
    if (n_unlike) *n_unlike = fi.n_unlike;
    const int rc = fq_finish(c, fn, in->max_reads, n_reads_out, !check_only);
    if (fi.status == FQ_OK || fi.status == FQ_E_EMPTY || fi.status == FQ_E_LONG || fi.status == FQ_E_OFFSETS) {      // the lines were found: the tails are known
        c->fq.tail_n[0] = p.n[0] - fi.tail_at[0]; c->fq.tail_n[1] = two ? p.n[1] - fi.tail_at[1] : 0;
        c->fq.tail_valid = true;
        if (tail) { tail[0] = c->fq.tail_n[0]; tail[1] = c->fq.tail_n[1]; }
    }
    if (rc == DG_OK && check_only) c->no_batch = true;
    return rc;
}

extern "C" int dg_batch_download_fastq_tail(dg_ctx *c, char *tail1, size_t cap1, char *tail2, size_t cap2)
{
    if (!c) return DG_ERR_ARG;
    if (!c->fq.tail_valid) { snprintf(c->err, 512, "dg_batch_download_fastq_tail: no tails (dg_batch_upload_fastq_bgzf first)"); return DG_ERR_ARG; }
    if (cap1 < c->fq.tail_n[0] || cap2 < c->fq.tail_n[1]) { snprintf(c->err, 512, "dg_batch_download_fastq_tail: output capacity too small (need %zu %zu)", c->fq.tail_n[0], c->fq.tail_n[1]); return DG_ERR_CAPACITY; }
    if ((c->fq.tail_n[0] && !tail1) || (c->fq.tail_n[1] && !tail2)) return DG_ERR_ARG;
    if (!c->fq.tail_n[0] && !c->fq.tail_n[1]) return DG_OK;
    HIPCHK(hipSetDevice(c->device));
    if (c->fq.tail_n[0]) HIPCHK(hipMemcpyAsync(tail1, c->fq.tail.p, c->fq.tail_n[0], hipMemcpyDeviceToHost, c->stream));
    if (c->fq.tail_n[1]) HIPCHK(hipMemcpyAsync(tail2, c->fq.tail.p + c->fq.tail_off2, c->fq.tail_n[1], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));
    return DG_OK;
}

extern "C" int dg_batch_fastq_device_ms(dg_ctx *c, float *ms)
{
    if (!c || !ms) return DG_ERR_ARG;
    *ms = c->fq.ms;
    return DG_OK;
}

// ------------------------------------------------------------------------------------------
// trimming inside the FASTQ upload (dg_trim.h)
// ------------------------------------------------------------------------------------------
extern "C" int dg_set_trim(dg_ctx *c, const dg_trim *t)
{
    if (!c) return DG_ERR_ARG;
    if (!t) { c->tr.on = false; return DG_OK; }
    if (t->flags & ~DG_TRIM_PAIRS) { snprintf(c->err, 512, "dg_set_trim: unknown flag bits 0x%x", t->flags & ~DG_TRIM_PAIRS); return DG_ERR_ARG; }
    if (t->min_len == 0 || t->min_overlap == 0) { snprintf(c->err, 512, "dg_set_trim: min_len and min_overlap must be at least 1"); return DG_ERR_ARG; }
    if (t->max_err_permille > 1000u) { snprintf(c->err, 512, "dg_set_trim: max_err_permille is %u, above 1000", t->max_err_permille); return DG_ERR_ARG; }
    if (t->poly_mask & ~15u) { snprintf(c->err, 512, "dg_set_trim: poly_mask 0x%x has a bit above 3", t->poly_mask); return DG_ERR_ARG; }
    if (t->qual3 > TR_QUAL_MAX || t->qual5 > TR_QUAL_MAX || t->qual_base > TR_QUAL_MAX) { snprintf(c->err, 512, "dg_set_trim: qual3, qual5 and qual_base must not exceed %u", TR_QUAL_MAX); return DG_ERR_ARG; }
    TrimPar par = {};
    for (int i = 0; i < 2; i++) {
        if (t->n_adapter[i] > 64u) { snprintf(c->err, 512, "dg_set_trim: adapter %d has %u bases, more than 64", i, t->n_adapter[i]); return DG_ERR_ARG; }
        for (uint32_t j = 0; j < t->n_adapter[i]; j++) {
            const char b = t->adapter[i][j];
            if (b != 'A' && b != 'C' && b != 'G' && b != 'T') { snprintf(c->err, 512, "dg_set_trim: adapter %d has a byte outside ACGT at %u", i, j); return DG_ERR_ARG; }
            par.acode[i][j >> 5] |= (uint64_t)trim_code(b) << (2u * (j & 31u));
        }
        par.alen[i] = t->n_adapter[i];
    }
    par.flags = t->flags; par.qual3 = t->qual3; par.qual5 = t->qual5; par.qual_base = t->qual_base; par.min_overlap = t->min_overlap; par.max_err_permille = t->max_err_permille;
    par.poly_mask = t->poly_mask; par.poly_min = t->poly_min; par.min_len = t->min_len;
    c->tr.par = par; c->tr.on = true;
    return DG_OK;
}

extern "C" int dg_set_umi(dg_ctx *c, const dg_umi *u)
{
    if (!c) return DG_ERR_ARG;
    if (!u) { c->tr.umi_on = false; return DG_OK; }
    if (u->flags & ~DG_UMI_PAIRS) { snprintf(c->err, 512, "dg_set_umi: unknown flag bits 0x%x", u->flags & ~DG_UMI_PAIRS); return DG_ERR_ARG; }
    if ((uint64_t)u->len[0] + u->len[1] == 0 || (uint64_t)u->len[0] + u->len[1] > UD_MAX_LEN) { snprintf(c->err, 512, "dg_set_umi: the two lengths together are %llu, not 1..%d", (unsigned long long)u->len[0] + u->len[1], UD_MAX_LEN); return DG_ERR_ARG; }
    for (int m = 0; m < 2; m++)
        if ((uint64_t)u->len[m] + u->skip[m] > (uint64_t)DG_MAX_RLEN) { snprintf(c->err, 512, "dg_set_umi: len[%d] + skip[%d] is %llu, above %d", m, m, (unsigned long long)u->len[m] + u->skip[m], DG_MAX_RLEN); return DG_ERR_ARG; }
    if (u->sep == 0 || u->sep == ' ' || u->sep == '\t' || u->sep == '/' || ud_code((unsigned char)u->sep)) { snprintf(c->err, 512, "dg_set_umi: the separator 0x%02x is NUL, a blank, a tab, '/' or one of ACGTN+-", (unsigned char)u->sep); return DG_ERR_ARG; }
    c->tr.umi = *u; c->tr.umi_on = true;
    return DG_OK;
}

extern "C" int dg_batch_trim_stats(dg_ctx *c, uint64_t stats[16], float *device_ms)
{
    if (!c || !stats) return DG_ERR_ARG;
    memcpy(stats, c->tr.stats, sizeof c->tr.stats);
    if (device_ms) *device_ms = c->tr.ms;
    return DG_OK;
}

extern "C" int dg_trim_granules(int out[2])
{
    if (!out) return DG_ERR_ARG;
    out[0] = FQ_THREADS; out[1] = 64;
    return DG_OK;
}

extern "C" int dg_batch_download_reads(dg_ctx *c, uint32_t *seq_off, uint16_t *rlen, char *seq, uint32_t *hdr_off, char *hdr, uint32_t *qual_off, char *qual,
                                       const size_t caps[3], size_t used[3])
{
    if (!c || !caps || !used) return DG_ERR_ARG;
    if (!c->fq.valid) { snprintf(c->err, 512, "dg_batch_download_reads: the context's last upload was not dg_batch_upload_fastq"); return DG_ERR_ARG; }
    used[0] = c->seq_bytes; used[1] = c->fq.hdr_bytes; used[2] = c->fq.qual_bytes;
    if (caps[0] < used[0] || caps[1] < used[1] || caps[2] < used[2]) { snprintf(c->err, 512, "dg_batch_download_reads: output capacity too small (need %zu %zu %zu)", used[0], used[1], used[2]); return DG_ERR_CAPACITY; }
    const size_t n = (size_t)c->n_reads;
    if (n == 0) { if (hdr_off) hdr_off[0] = 0; if (qual_off) qual_off[0] = 0; return DG_OK; }
    if (!seq_off || !rlen || !hdr_off || !qual_off || (used[0] && !seq) || (used[1] && !hdr) || (used[2] && !qual)) return DG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(seq_off, c->seq_off.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(rlen, c->rlen.p, n * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(hdr_off, c->fq.hdr_off.p, (n + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(qual_off, c->fq.qual_off.p, (n + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    if (used[0]) HIPCHK(hipMemcpyAsync(seq, c->seq.p, used[0], hipMemcpyDeviceToHost, c->stream));
    if (used[1]) HIPCHK(hipMemcpyAsync(hdr, c->fq.hdr.p, used[1], hipMemcpyDeviceToHost, c->stream));
    if (used[2]) HIPCHK(hipMemcpyAsync(qual, c->fq.qual.p, used[2], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));
    return DG_OK;
}

extern "C" void *dg_host_alloc(size_t bytes)
{
    void *p = nullptr;
    return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}
extern "C" void dg_host_free(void *p) { if (p) (void)hipHostFree(p); }

static WSLayout make_ws_layout(int R)
{
    WSLayout L;
    auto al = [](uint32_t x) { return (x + 15u) & ~15u; };
    uint32_t o = 0;
    const uint32_t nmax = 2u * (uint32_t)R + 32u;                       // longest genome fragment of a segment pair
    L.max_rlen = (uint32_t)R;
    L.cig_off = o; L.cig_cap = 4u * (uint32_t)R + 64u; o = al(o + L.cig_cap * 4u);
    L.nwbits_off = o; L.nwbits_words = ((uint32_t)R + 1u) * ((nmax + 7u) / 8u); o = al(o + L.nwbits_words * 4u);
    L.rows_off = o; L.row_cap = (uint32_t)R + 8u; o = al(o + 2u * L.row_cap * 4u);          // strip boundary column: s and r per row
    L.str_off = o; L.str_cap = al(3u * (uint32_t)R + 64u); o = al(o + 6u * L.str_cap);
    L.kmer_off = o; L.kmer_cap = (uint32_t)R + 8u > 48u ? (uint32_t)R + 8u : 48u; o = al(o + L.kmer_cap * 8u);   // also holds 4 x (4 + 6) u64 of pair strings/results
    uint32_t rd = 64; while (rd < (uint32_t)R + 1u) rd <<= 1;
    L.ring_diag = rd; L.ring_words = ((uint32_t)R + 64u) / 64u; L.ring_off = o; o = al(o + rd * L.ring_words * 8u);
    L.stride = (o + 255u) & ~255u;
    return L;
}

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the function on a device, not to a context: it only ever grows here (a
// context with shorter reads used to lower what a sibling with longer reads had set, whose next launch then asked for more than allowed)
#define DG_MAX_DEVICES 64
static std::mutex g_lds_mu;
static size_t g_lds_set[2][DG_MAX_DEVICES];
static hipError_t raise_dynamic_lds(const void *fn, int which, int device, size_t lds)
{
    std::lock_guard<std::mutex> lk(g_lds_mu);
    size_t &cur = g_lds_set[which][device & (DG_MAX_DEVICES - 1)];
    if (lds <= cur) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) cur = lds;
    return e;
}

// k_encode + k_seed (reads staged in LDS when 256 lanes x W words fit comfortably)
static hipError_t launch_seed(dg_ctx *c, int n, int H, hipEvent_t after_encode = nullptr)
{
    const int W = 2 * ((c->max_rlen + 15) / 16 > 0 ? (c->max_rlen + 15) / 16 : 1);   // 2-bit words + N-mask words per read
    hipError_t e = c->enc.ensure((size_t)W * n + 16);
    if (e != hipSuccess) return e;
    int lg = 0;
    while ((1 << lg) < W / 2) lg++;
    if (!c->enc_ready) k_encode<<<(unsigned)((((size_t)n << lg) + 255) / 256), 256, 0, c->stream>>>(c->seq.p, c->seq_off.p, c->rlen.p, n, W, lg, c->enc.p);
    if (after_encode) { e = hipEventRecord(after_encode, c->stream); if (e != hipSuccess) return e; }
    // persistent one-wave workgroups pulling reads from a queue (TOP_SEED_NEXT); long walks go to TOP_SEED_HEAVY's list
    if ((e = c->seed_heavy.ensure((size_t)n + 16)) != hipSuccess) return e;
    unsigned blocks = (unsigned)c->n_cu * (unsigned)c->env_seed_waves;   // one wave per SIMD: the kernel is instruction-fetch bound, more waves add ~10 % alone but cost more than
                                                                         // that to the other batches in flight (measured 5.4 vs 6.0 ms per step with four batches)
    if ((size_t)blocks * 64 > (size_t)n) blocks = (unsigned)((n + 63) / 64);
    const bool use_qf = !c->env_seed_legacy && !c->env_seed_phases && W <= 62 && c->pr.max_dup <= 30000;      // (k_seed_qf's slot state counts occurrences in 20 bits: 31 hits x max_dup)
    const int bail_trips = c->env_bail_trips > 0 ? c->env_bail_trips : (use_qf ? 64 : 128);
    unsigned int *tops = c->d_tops;
    // default: the queue kernel (dg_seedq.h).  DG_SEED_LEGACY=1 or reads too long for its LDS slots (> 496 bases): the lane-per-read kernel
    c->seed_qf_used = false;
    if (use_qf) {
        // the free-running queue kernel (dg_seedq.h, k_seed_qf): workgroups of `nw` waves around 2^lg read slots
        int lg = c->env_seed_slots_lg >= 6 && c->env_seed_slots_lg <= 11 ? c->env_seed_slots_lg : 9;
        int nw = c->env_seed_wg_waves >= 1 && c->env_seed_wg_waves <= 8 ? c->env_seed_wg_waves : 4;
        while (lg > 6 && sqf_lds_bytes(lg, W, nw) > (size_t)156 * 1024) lg--;
        if (c->env_seed_slots_lg == 0) while (lg > 6 && sqf_lds_bytes(lg, W, nw) > (size_t)80 * 1024) lg--;      // default: two workgroups per CU
        const size_t lds = sqf_lds_bytes(lg, W, nw);
        if ((e = raise_dynamic_lds((const void *)k_seed_qf, 0, c->device, lds)) != hipSuccess) return e;
        unsigned per_cu = (unsigned)(((size_t)160 * 1024) / lds);
        if (per_cu * (unsigned)nw > 16u) per_cu = 16u / (unsigned)nw;
        // Two workgroups per CU although three fit: the launch lasts as long as its slowest reads' chains of trips whatever the number of waves
        // (alone 0.98 ms with two or three), and the third workgroup's 50 KB of LDS is what another batch's k_pair (72 KB) needs to start on
        // the same CU: 840 against 806 M reads/s with twelve batches in flight (profiles/r03/d_variants_wgs_per_cu.txt).  DG_SEED_WGS overrides.
        if (per_cu > 2u) per_cu = 2u;
        if (per_cu < 1u) per_cu = 1u;
        if (c->env_seed_wgs > 0) per_cu = (unsigned)c->env_seed_wgs;
        unsigned wgs = (unsigned)c->n_cu * per_cu;
        const unsigned need = (unsigned)(((size_t)n + ((size_t)1 << lg) - 1) >> lg);
        if (wgs > need) wgs = need;
        c->seed_qf_used = true;
        k_seed_qf<<<wgs, nw * 64, lds, c->stream>>>(c->ix, c->pr, c->enc.p, c->rlen.p, n, W, H, lg, c->hits.p, c->nhits.p, c->nseeds.p, tops + TOP_SEED_NEXT,
                                                    c->seed_heavy.p, tops + TOP_SEED_HEAVY, c->d_ctr, bail_trips, c->env_seed_partial, c->env_seed_multi, c->d_err, bail_trips);
    } else
    if (!c->env_seed_legacy && W <= 62) {
        int lg = c->env_seed_slots_lg >= 6 && c->env_seed_slots_lg <= 10 ? c->env_seed_slots_lg : 9;
        while (lg > 6 && sq_lds_bytes(lg, W) > (size_t)80 * 1024) lg--;
        const size_t lds = sq_lds_bytes(lg, W);
        if ((e = raise_dynamic_lds((const void *)k_seed_q, 1, c->device, lds)) != hipSuccess) return e;
        unsigned per_cu = (unsigned)(((size_t)160 * 1024) / lds);
        if (per_cu > 4u) per_cu = 4u;
        if (c->env_seed_wgs > 0) per_cu = (unsigned)c->env_seed_wgs;
        unsigned wgs = (unsigned)c->n_cu * per_cu;
        const unsigned need = (unsigned)(((size_t)n + ((size_t)1 << lg) - 1) >> lg);
        if (wgs > need) wgs = need;
        k_seed_q<<<wgs, SQ_THREADS, lds, c->stream>>>(c->ix, c->pr, c->enc.p, c->rlen.p, n, W, H, lg, c->hits.p, c->nhits.p, c->nseeds.p, tops + TOP_SEED_NEXT,
                                                      c->seed_heavy.p, tops + TOP_SEED_HEAVY, c->d_ctr, bail_trips, c->d_err);
    } else
    if (W <= 78) k_seed<true><<<blocks, 64, ((size_t)2 * W * 64 + 64) * 4, c->stream>>>(c->ix, c->pr, c->enc.p, c->rlen.p, n, W, H, c->hits.p, c->nhits.p, c->nseeds.p, tops + TOP_SEED_NEXT, c->seed_heavy.p, tops + TOP_SEED_HEAVY, c->d_ctr, bail_trips);
    else k_seed<false><<<blocks, 64, 0, c->stream>>>(c->ix, c->pr, c->enc.p, c->rlen.p, n, W, H, c->hits.p, c->nhits.p, c->nseeds.p, tops + TOP_SEED_NEXT, c->seed_heavy.p, tops + TOP_SEED_HEAVY, c->d_ctr, bail_trips);
    // the backward walk of every listed read, lane = read (dg_fm.h): from which start on all searches fail without being made
    if ((e = c->seed_heavy_sfail.ensure((size_t)n + 16)) != hipSuccess) return e;
    k_seed_heavy_walk<<<(unsigned)c->n_cu * 8u, 64, 0, c->stream>>>(c->ix, c->pr, c->enc.p, c->rlen.p, W, c->seed_heavy.p, tops + TOP_SEED_HEAVY, c->seed_heavy_sfail.p, c->d_ctr);
    k_seed_heavy<<<(unsigned)c->n_cu * (unsigned)c->env_seedh_bpc, 64, (size_t)W * 4 + 16, c->stream>>>(c->ix, c->pr, c->enc.p, c->rlen.p, W, H, c->hits.p, c->nhits.p, c->nseeds.p, c->seed_heavy.p, tops + TOP_SEED_HEAVY, c->seed_heavy_sfail.p, c->d_ctr);
    return hipGetLastError();
}

// A look-back may wait ~2 s of wall clock for a predecessor (DG_SCAN_POLL_BUDGET, the tests' hook: a poll count on a batch's FIRST attempt instead).
// `first_tile`: where this scan's tiles start in the context's state / trace arrays.
static TileScan make_tile_scan(dg_ctx *c, size_t first_tile, unsigned int *ticket, int which /* 1 = seed offsets, 2 = k_pair, 4 = k_emit_slow: DG_SCAN_POLL_SCANS picks the hooked ones */)
{
    TileScan ts;
    ts.w = c->scan_state.p + SCAN_WORDS * first_tile; ts.ticket = ticket; ts.epoch = c->scan_epoch;
    ts.budget = (c->env_scan_budget > 0 && c->attempt_no == 0 && (c->env_scan_mask & which)) ? (uint32_t)c->env_scan_budget : 0u;
    ts.dbg = c->d_sizes->scan_dbg;
    ts.ticks = (unsigned long long)c->wall_khz * 2000ull;
    ts.trace = c->scan_trace.p ? c->scan_trace.p + SCAN_TRACE_WORDS * first_tile : nullptr;
    return ts;
}

#define TICK(name) do { if (c->n_t < N_TIMERS) { c->tname[c->n_t] = name; HIPCHK(hipEventRecord(c->ev[c->n_t + 1], c->stream)); c->n_t++; } } while (0)

// the kernels of the seeding + locate stage up to the located, unsorted seeds (shared by dg_batch_run and dg_probe_seeds)
static int enqueue_seeding(dg_ctx *c, int n, int H, bool timed, bool paired_units)
{
    HIPCHK(c->hits.ensure((size_t)n * H)); HIPCHK(c->nhits.ensure(n)); HIPCHK(c->nseeds.ensure(n)); HIPCHK(c->seed_off.ensure((size_t)n + 1));
    if (c->shared_caps) caps_adopt(c->cap_seeds, c->shared_caps->seeds);
    if (c->cap_seeds < (size_t)n * 3 + 1024) c->cap_seeds = (size_t)n * 3 + 1024;              // first guess: ~2.5 seeds per read; grows by itself
    HIPCHK(c->seeds.ensure(c->cap_seeds + 1)); HIPCHK(c->cands.ensure(c->cap_seeds + 1)); HIPCHK(c->tile_read.ensure(c->cap_seeds / 64 + 16));
    if (timed) c->tname[c->n_t] = "k_encode";
    HIPCHK(launch_seed(c, n, H, timed ? c->ev[c->n_t + 1] : nullptr));
    if (timed) { c->n_t++; TICK("k_seed"); }
    {
        const int paired = (paired_units && (n % 2 == 0)) ? 1 : 0;
        HIPCHK(c->heavy.ensure((size_t)n + 16));
        const TileScan ts_seed = make_tile_scan(c, 0, c->d_tops + TOP_TICKET_SEED, 1);
        k_seed_offsets<<<(unsigned)((n + 256 * SO_PER - 1) / (256 * SO_PER)), 256, 0, c->stream>>>(n, paired, c->nseeds.p, c->seed_off.p, c->tile_read.p, (uint32_t)c->tile_read.cap,
                                                                                                 c->heavy.p, c->d_tops + TOP_HEAVY_UNITS, &c->d_sizes->total_seeds, (uint32_t)c->cap_seeds, ts_seed, c->d_err);
        HIPCHK(hipGetLastError());
    }
    if (timed) TICK("seed_offsets");
    k_locate<<<(unsigned)((c->cap_seeds + 255) / 256), 256, 0, c->stream>>>(c->ix, n, H, c->hits.p, c->tile_read.p, c->seed_off.p, c->seeds.p, c->d_ctr, c->d_err);
    HIPCHK(hipGetLastError());
    if (timed) TICK("k_locate");
    return DG_OK;
}

// the small per-batch state -- work counters, bump tops and tickets, status word, sizes -- zeroed by ONE launch (round 2: five fills;
// the four blocks stay separate allocations: the status word every workgroup reads must not share lines with the tops every workgroup bumps)
__global__ void __launch_bounds__(256)
k_batch_begin(unsigned long long *ctr, unsigned int *tops, int *err, DSizes *sizes)
{
    for (int i = threadIdx.x; i < CTR_STRIPES * CTR_STRIDE; i += 256) ctr[i] = 0ull;
    if (threadIdx.x < N_TOPS) tops[threadIdx.x] = 0u;
    if (threadIdx.x < (int)(sizeof(DSizes) / 4)) ((uint32_t *)sizes)[threadIdx.x] = 0u;
    if (threadIdx.x == 0) *err = 0;
}

// the look-back state of the batch's three single-pass scans in c->scan_state: [seed offsets | k_pair | k_emit_slow]
static size_t scan_tiles_seed(int n_reads) { return (size_t)(n_reads + 256 * SO_PER - 1) / (256 * SO_PER) + 1; }
static size_t scan_tiles_pair(int n_units) { return (size_t)(n_units + PU_THREADS - 1) / PU_THREADS + 1; }

// the tail of a batch: sizes, status word, tops and the work counters (their 64 stripes summed -- or, for the two maxima, maximised -- here)
// written straight into the context's page-locked host block by ONE launch (round 2: four device-to-host copies) -- and, since round 5, left ZEROED for
// the next run of the context, which then needs no k_batch_begin in front (one launch per batch less; every thread clears what it has just read)
__global__ void __launch_bounds__(256)
k_batch_end(DSizes *__restrict__ sizes, int *__restrict__ err, unsigned int *__restrict__ tops, unsigned long long *__restrict__ ctr, dg_ctx::HostTail *out)
{
    const int t = threadIdx.x;
    if (t < (int)(sizeof(DSizes) / 4)) { out->sizes_words()[t] = ((const uint32_t *)sizes)[t]; ((uint32_t *)sizes)[t] = 0u; }
    if (t < N_TOPS) { out->tops[t] = tops[t]; tops[t] = 0u; }
    if (t == 0) { out->err = *err; *err = 0; }
    if (t < CTR_STRIDE) {
        const bool is_max = t == CTR_MAXTRIPS || t == CTR_WTRIPS_MAX;
        unsigned long long v = 0;
        for (int s_ = 0; s_ < CTR_STRIPES; s_++) { const unsigned long long x = ctr[s_ * CTR_STRIDE + t]; ctr[s_ * CTR_STRIDE + t] = 0ull; v = is_max ? (x > v ? x : v) : v + x; }
        out->ctr[t] = v;
    }
}

static int zero_batch_state(dg_ctx *c, int n_reads, int n_units)
{
    if (!c->state_zeroed) {                     // (a context's first run, or the run after one whose enqueue failed half-way: k_batch_end of every complete run leaves the state zeroed)
        k_batch_begin<<<1, 256, 0, c->stream>>>(c->d_ctr, c->d_tops, c->d_err, c->d_sizes);
        HIPCHK(hipGetLastError());
    }
    c->state_zeroed = false;
    // the look-back state of the two single-pass scans is NOT zeroed per batch: its words carry the run's epoch (dg_scan.h).
    // Zeroed once, when (re)allocated: epoch 0 is never used.
    const size_t tiles2 = (size_t)(2 * n_units + 255) / 256 + 1;
    const size_t words = SCAN_WORDS * (scan_tiles_seed(n_reads) + scan_tiles_pair(n_units) + tiles2);
    if (words > c->scan_state.cap) {
        HIPCHK(c->scan_state.ensure(words));
        HIPCHK(hipMemsetAsync(c->scan_state.p, 0, c->scan_state.cap * 8, c->stream));
        static_assert(SCAN_TRACE_WORDS == SCAN_WORDS, "the trace array is sized like the state array");
        HIPCHK(c->scan_trace.ensure(c->scan_state.cap));
        HIPCHK(hipMemsetAsync(c->scan_trace.p, 0, c->scan_trace.cap * 8, c->stream));
    }
    c->scan_epoch = (c->scan_epoch + 1u) & 0x3FFFFFFFu;
    if (c->scan_epoch == 0) c->scan_epoch = 1;
    return DG_OK;
}


// Enqueues the whole path of the uploaded batch on the context's stream and returns without waiting: no size is read back
// in between.  finish_run() waits, learns the sizes, and runs the batch again if a capacity was too small.
static int enqueue_run(dg_ctx *c)
{
    const int n = c->n_reads;
    const int paired = (c->pr.paired && (n % 2 == 0)) ? 1 : 0;      // Mapping.cpp:598
    const int n_units = paired ? n / 2 : n;
    refresh_index(c);
    c->n_t = 0;
    const int H = c->max_rlen / 16 + 1;
    const uint32_t nb = (uint32_t)((n + 255) / 256);
    { const int zr = zero_batch_state(c, n, n_units); if (zr) return zr; }
    HIPCHK(hipEventRecord(c->ev[0], c->stream));
    { const int rc = enqueue_seeding(c, n, H, true, c->pr.paired != 0); if (rc) return rc; }

    // capacities of the data-dependent buffers (sticky; see dg_ctx)
    if (c->shared_caps) { caps_adopt(c->cap_rep, c->shared_caps->rep); caps_adopt(c->cap_cig, c->shared_caps->cig); caps_adopt(c->cap_work, c->shared_caps->work); }
    if (c->cap_rep < (size_t)n + (size_t)n / 4 + 1024) c->cap_rep = (size_t)n + (size_t)n / 4 + 1024;
    if (c->cap_cig < 3 * c->cap_rep) c->cap_cig = 3 * c->cap_rep;
    if (c->cap_work < (size_t)n * 8 + 65536) c->cap_work = (size_t)n * 8 + 65536;
    const size_t cigcap = (size_t)n * 48 + c->cap_rep * (16 + CIG_SLOT) + 4096, sjcap = (size_t)n * 4 + 1024;
    HIPCHK(c->ncand.ensure(n)); HIPCHK(c->rep_off.ensure((size_t)n + 1)); HIPCHK(c->reads_out.ensure(n));
    HIPCHK(c->heavy.ensure((size_t)n_units + 16)); HIPCHK(c->slow_units.ensure((size_t)n_units + 16));
    HIPCHK(c->reports.ensure(c->cap_rep + 1)); HIPCHK(c->work.ensure(c->cap_work + 16)); HIPCHK(c->jobs.ensure(c->cap_seeds + 16));
    // k_reseed's work list: (window, chunk) items per ring size, and one record per chunk of the windows that several waves share (dg_reseed.h)
    const uint32_t rs_out_cap = (uint32_t)std::max<size_t>(16384, (size_t)n / 8), rs_list_cap = (uint32_t)std::min<size_t>(c->jobs.cap + rs_out_cap, 0xFFFFFFF0u);
    HIPCHK(c->job_outs.ensure(rs_out_cap)); HIPCHK(c->job_items.ensure(3 * (size_t)rs_list_cap + 16));
    const uint32_t rs_pool_cap = (uint32_t)std::max<size_t>(16384, (size_t)n / 32);           // blocks of 64 entries for the chunks that report more than their record holds
    HIPCHK(c->job_pool.ensure((size_t)rs_pool_cap * 64)); HIPCHK(c->job_pool_next.ensure(rs_pool_cap));
    HIPCHK(c->cigpool.ensure(cigcap)); HIPCHK(c->cigfinal.ensure(c->cap_cig + 16)); HIPCHK(c->sjpool.ensure(sjcap)); HIPCHK(c->sjfinal.ensure(sjcap));
    HIPCHK(c->items.ensure(c->cap_seeds + 16));                 // k_report's work list: one item per live candidate of the general path (candidates <= seeds)
    unsigned int *tops = c->d_tops;

    // units with more seeds than a lane of k_pair holds: a wave each, before k_pair (which needs their candidate counts)
    HIPCHK(c->chain_picks.ensure(c->cap_seeds + 16)); HIPCHK(c->chain_todo.ensure((size_t)n_units + 16));
    k_chain_heavy<<<c->n_cu * c->env_chain_bpc, 64, 0, c->stream>>>(c->ix, c->pr, n_units, paired, c->rlen.p, c->seed_off.p, c->seeds.p, c->cands.p, c->ncand.p,
                                                     c->heavy.p, tops + TOP_HEAVY_UNITS, c->chain_picks.p, c->chain_todo.p, c->d_ctr, c->d_err);
    // the sequential rest of the candidate rules of those units, lane = unit (dg_chain.h)
    k_chain_rules<<<c->n_cu * 4, 64, 0, c->stream>>>(paired, c->seed_off.p, c->cands.p, c->ncand.p, c->heavy.p, tops + TOP_HEAVY_UNITS, c->chain_picks.p, c->chain_todo.p, c->d_err);
    HIPCHK(hipGetLastError());
#ifdef DG_PROFILE_CLASSES
    {
        unsigned long long v[3], z = 0;
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpyFromSymbol(&v[0], HIP_SYMBOL(g_chain_max), 8)); HIPCHK(hipMemcpyFromSymbol(&v[1], HIP_SYMBOL(g_chain_units), 8)); HIPCHK(hipMemcpyFromSymbol(&v[2], HIP_SYMBOL(g_chain_cycles), 8));
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_chain_max), &z, 8)); HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_chain_units), &z, 8)); HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_chain_cycles), &z, 8));
        fprintf(stderr, "[chain_heavy] units %llu  mean cycles %llu  max cycles %llu (seeds %llu/%llu cands %llu/%llu)\n", v[1], v[1] ? v[2] / v[1] : 0, v[0] >> 40,
                (v[0] >> 30) & 1023, (v[0] >> 20) & 1023, (v[0] >> 10) & 1023, v[0] & 1023);
    }
#endif
    TICK("k_chain_heavy");
    const size_t tiles_s = scan_tiles_seed(n), tiles = scan_tiles_pair(n_units);
    const TileScan ts_pair = make_tile_scan(c, tiles_s, tops + TOP_TICKET_PAIR, 2), ts_emit = make_tile_scan(c, tiles_s + tiles, tops + TOP_TICKET_EMIT, 4);
    const int try_fast = (c->env_no_fast || c->ix.n_chr > 0xFFFF) ? 0 : 1;
    // the compact record types are written by the kernels that write the full ones (unless the caller is known to take the full ones: dg_map_batch)
    CompactOut co{nullptr, nullptr, nullptr, nullptr};
    if (c->want_compact) {
        HIPCHK(c->reads_c.ensure((size_t)n + 1)); HIPCHK(c->reports_c.ensure(c->cap_rep + 1)); HIPCHK(c->cig_c.ensure(c->cap_cig + 16));
        co = CompactOut{c->reads_c.p, c->reports_c.p, c->cig_c.p, &c->d_sizes->pad[1]};
    }
    const int W2p = (c->max_rlen + 15) / 16 > 0 ? (c->max_rlen + 15) / 16 : 1;
    const bool packed_pair = c->enc_ready;        // a packed batch: the characters follow from its words; only the general path's units get an ASCII copy (below)
    auto launch_pair = [&](auto kernel) {
        kernel<<<(unsigned)((n_units + PU_THREADS - 1) / PU_THREADS), PU_THREADS, 0, c->stream>>>(
            c->ix, c->pr, n_units, paired, try_fast, (c->want_full || !c->want_compact) ? 0 : 2, c->seq.p, c->seq_off.p, c->enc.p, W2p, c->rlen.p, c->seed_off.p, c->seeds.p, c->cands.p, c->ncand.p, c->rep_off.p,
            c->slow_units.p, c->reads_out.p, c->reports.p, c->cigfinal.p, (uint32_t)c->cap_rep, (uint32_t)c->cap_cig, ts_pair, c->d_sizes, tops + TOP_CIG, c->d_ctr, c->d_err, co);
    };
    if (packed_pair) launch_pair(k_pair<true>); else launch_pair(k_pair<false>);
    HIPCHK(hipGetLastError());
    TICK("k_pair");

    // ---- the general path, on the units k_pair listed ----
    const WSLayout L = make_ws_layout(c->max_rlen < 32 ? 32 : c->max_rlen);
    int blocks = c->n_cu * c->env_report_bpc;       // 8 one-wave workgroups per CU (2 per SIMD: the kernel needs ~220 VGPRs to stay out of scratch)
    if ((size_t)blocks * 64 > (size_t)n) blocks = (n + 63) / 64;
    {   // the lane workspace grows with the square of the longest read: keep it under ~12 GB by running fewer persistent waves
        const size_t budget = (size_t)12 << 30, per_block = (size_t)64 * L.stride;
        if ((size_t)blocks * per_block > budget) blocks = (int)(budget / per_block);
        if (blocks < 1) blocks = 1;
    }
    HIPCHK(c->ws.ensure((size_t)blocks * 64 * L.stride));
    unsigned slow_grid = (unsigned)c->n_cu * 4u;
    if ((size_t)slow_grid * 256 > (size_t)n) slow_grid = nb;
    k_prep<dg_report_out><<<slow_grid, 256, 0, c->stream>>>(c->pr, paired, c->slow_units.p, c->d_sizes, c->seed_off.p, c->seeds.p, c->cands.p, c->ncand.p, c->work.p, tops + TOP_WORK,
                                             (uint32_t)c->cap_work, c->jobs.p, tops + TOP_JOBS, (uint32_t)c->jobs.cap, c->d_err, c->rlen.p, c->rep_off.p, c->reports.p, tops + TOP_CLASS_HIST,
                                             packed_pair ? c->enc.p : nullptr, W2p, c->seq.p);      // (a packed batch: the listed reads get their ASCII copy here)
    HIPCHK(hipGetLastError());
    TICK("k_prep");
    // The re-seeding kernels run on the context's only stream, before the report kernel, which then takes ALL candidates in one launch.  Rounds 1-4
    // gave a wave a whole window (up to 500 kb = ~1000 serial trips): the kernel was one long tail, so it ran on a second stream beside the report of the
    // candidates without jobs -- whose persistent waves held 113 of a CU's 160 KB of LDS and left k_reseed three waves per CU (cfg5: 3.8 s of wave time in
    // 5.4 ms).  With windows shared by several waves (dg_reseed.h) it is a balanced throughput kernel that wants the GPU for itself for a short time; a
    // context owns ONE stream (the sixteen hardware queues of a process hold twelve contexts, the caller's stream and -- on a node -- RCCL's).
    const uint32_t jobcap = (uint32_t)c->jobs.cap;
    const RsPool rs_pool{c->job_pool.p, c->job_pool_next.p, tops + TOP_RS_POOL, c->env_rs_pool > 0 ? std::min<uint32_t>((uint32_t)c->env_rs_pool, rs_pool_cap) : rs_pool_cap};
    const int rs_gap_max = c->max_rlen - 32, rs_need = rs_gap_max >= 8 ? (rs_gap_max - 8) / 64 + 1 : 1;        // (see below)
    // k_order: k_reseed's work list ((window, chunk) items per ring size) and k_report's (the candidates grouped by cost class)
    const RsOrder rs_order{c->jobs.p, tops + TOP_JOBS, jobcap, c->job_items.p, rs_list_cap, rs_out_cap, rs_need <= 1 ? 1 : (rs_need <= 2 ? 2 : 4), (uint32_t)c->env_rs_chunk, tops + TOP_RESEED_COUNT, tops + TOP_RS_OUT};
    k_order<<<slow_grid, 256, 0, c->stream>>>(paired, c->slow_units.p, c->d_sizes, c->seed_off.p, c->cands.p, c->ncand.p, tops + TOP_CLASS_HIST, tops + TOP_CLASS_FILL, c->items.p, tops + TOP_ORDER_INFO, rs_order, c->d_err);
    HIPCHK(hipGetLastError());
    TICK("order");
    // One launch per ring size the batch can need: a read gap lies between two seeds of >= 16 bases (bwt_search.cpp:165), so it is at most rlen - 32 long and
    // needs (gap - 16) / 64 + 1 bitmap words per diagonal -- one for reads of up to 103 bases (round 4 launched all three sizes for every batch), two up to 167.
    // (one stream for the ring sizes: side by side on streams of their own they cost the step 8 % with eight batches in flight, profiles/r02)
    k_reseed<1><<<c->n_cu * 10 * c->env_reseed_pct / 100, 64, 0, c->stream>>>(c->ix, c->seq.p, c->seq_off.p, c->jobs.p, c->job_items.p, tops + TOP_RESEED_COUNT, tops + TOP_RESEED_COUNT + 3, tops + TOP_RESEED_TICKET, c->job_outs.p, rs_pool, c->env_rs_inline, c->d_ctr, c->d_err);
    if (rs_need > 1) k_reseed<2><<<c->n_cu * 6 * c->env_reseed_pct / 100, 64, 0, c->stream>>>(c->ix, c->seq.p, c->seq_off.p, c->jobs.p, c->job_items.p + rs_list_cap, tops + TOP_RESEED_COUNT + 1, tops + TOP_RESEED_COUNT + 3, tops + TOP_RESEED_TICKET + 1, c->job_outs.p, rs_pool, c->env_rs_inline, c->d_ctr, c->d_err);
    if (rs_need > 2) k_reseed<4><<<c->n_cu * 4 * c->env_reseed_pct / 100, 64, 0, c->stream>>>(c->ix, c->seq.p, c->seq_off.p, c->jobs.p, c->job_items.p + 2 * (size_t)rs_list_cap, tops + TOP_RESEED_COUNT + 2, tops + TOP_RESEED_COUNT + 3, tops + TOP_RESEED_TICKET + 2, c->job_outs.p, rs_pool, c->env_rs_inline, c->d_ctr, c->d_err);
    HIPCHK(hipGetLastError());
    TICK("k_reseed");
    const uint32_t *n_items_p = tops + TOP_ORDER_INFO + 1;            // end of k_order's item list
    k_report<2><<<blocks, 64, 0, c->stream>>>(c->ix, c->pr, n, paired, c->seq.p, c->seq_off.p, c->rlen.p, c->seed_off.p, c->jobs.p, c->cands.p,
                                               c->rep_off.p, c->work.p, c->items.p, n_items_p, c->reports.p, c->cigpool.p,
                                               (uint32_t)cigcap, tops, c->ws.p, L, c->d_ctr, c->d_err);
    HIPCHK(hipGetLastError());
#ifdef DG_PROFILE_CLASSES
    {
        unsigned long long cyc[DG_COST_CLASSES + 1], cnt[DG_COST_CLASSES + 1], z[DG_COST_CLASSES + 1] = {0};
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpyFromSymbol(cyc, HIP_SYMBOL(g_class_cycles), sizeof cyc)); HIPCHK(hipMemcpyFromSymbol(cnt, HIP_SYMBOL(g_class_chunks), sizeof cnt));
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_class_cycles), z, sizeof z)); HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_class_chunks), z, sizeof z));
        unsigned long long tot = 0; for (int k = 0; k <= DG_COST_CLASSES; k++) tot += cyc[k];
        unsigned long long ph[DG_NCLS][DG_NPHASE], zp[DG_NCLS][DG_NPHASE] = {{0}};
        HIPCHK(hipMemcpyFromSymbol(ph, HIP_SYMBOL(g_phase), sizeof ph)); HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_phase), zp, sizeof zp));
        for (int k = 0; k < DG_COST_CLASSES; k++) if (cnt[k]) {
            fprintf(stderr, "[class %2d] chunks %7llu  cycles/chunk %8llu  share %5.1f %%  phases/chunk:", k, cnt[k], cyc[k] / cnt[k], 100.0 * cyc[k] / (tot ? tot : 1));
            for (int q = 0; q < DG_NPHASE; q++) fprintf(stderr, " %llu", ph[k][q] / cnt[k]);
            fprintf(stderr, "\n");
        }
    }
#endif
    TICK("k_report");
    k_finalize<<<slow_grid, 256, 0, c->stream>>>(c->ix, c->pr, paired, c->slow_units.p, c->d_sizes, c->seed_off.p, c->cands.p, c->ncand.p, c->rep_off.p, c->work.p,
                                                 c->reads_out.p, c->reports.p, c->sjpool.p, (uint32_t)sjcap, tops, c->d_err);
    k_emit_slow<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(paired, c->slow_units.p, c->d_sizes, c->reads_out.p, c->reports.p, c->cigpool.p, c->cigfinal.p,
                                                                    (uint32_t)c->cap_cig, c->sjpool.p, c->sjfinal.p, ts_emit, c->d_err, c->rlen.p, co);
    HIPCHK(hipGetLastError());
    TICK("k_finalize");
    // the tail: sizes, status, counters -> pinned host memory, one copy each
    k_batch_end<<<1, 256, 0, c->stream>>>(c->d_sizes, c->d_err, c->d_tops, c->d_ctr, c->h_tail);
    HIPCHK(hipGetLastError());
    c->state_zeroed = true;
    TICK("tail");
    c->enqueued = true;
    return DG_OK;
}

// waits for the enqueued batch; on a capacity overflow grows the buffer from what the device reported and runs the batch again
static int finish_run(dg_ctx *c, size_t used[3])
{
    c->runs_of_last_batch = 0;
    for (int attempt = 0; attempt < 6; attempt++) {
        c->runs_of_last_batch++;
        HIPCHK(wait_stream(c));
        if (c->enc_ready && c->h_tail->input_bad) { snprintf(c->err, 512, "packed batch: the N list holds a position outside the batch"); c->enqueued = false; return DG_ERR_ARG; }
        const DSizes &sz = c->h_tail->sizes;
        const int derr = c->h_tail->err;
        if (derr < DG_ABORT) break;
        auto grow = [](size_t need) { return need + need / 4 + 1024; };
        if (derr == DG_E_SEEDS) c->cap_seeds = grow(sz.total_seeds);
        else if (derr == DG_E_REPORTS) {        // (never shrinks: should the reported total ever be short, doubling still converges)
            c->cap_rep = std::max(grow(sz.total_rep), 2 * c->cap_rep);
            if (c->cap_cig < 3 * c->cap_rep) c->cap_cig = 3 * c->cap_rep;
        }
        else if (derr == DG_E_WORK) c->cap_work = grow(c->h_tail->tops[TOP_WORK]);
        else if (derr == DG_E_CIGFINAL) c->cap_cig = grow(sz.total_cig > 2 * c->cap_cig ? sz.total_cig : 2 * c->cap_cig);
        if (c->shared_caps) { caps_publish(c->shared_caps->seeds, c->cap_seeds); caps_publish(c->shared_caps->rep, c->cap_rep); caps_publish(c->shared_caps->work, c->cap_work); caps_publish(c->shared_caps->cig, c->cap_cig); }
        if (derr == DG_E_SEEDS || derr == DG_E_REPORTS || derr == DG_E_WORK || derr == DG_E_CIGFINAL) { /* grown above */ }
        else if ((derr == DG_E_SCAN || derr == DG_E_SEEDQ) && attempt < 5) {
            // a look-back that ran out of its time budget (dg_scan.h) or the seeding kernel's safety net: nothing to grow, the batch runs again (up to
            // five times: an event is rare -- three in 600 000 batches -- and independent of the batch) -- but never silently: what the poller saw and
            // what the stuck tile's workgroup last said about itself go to stderr and into the context's error text, the count into dg_last_counters [40]
            c->reruns_scan++;
            const unsigned long long *d = sz.scan_dbg;
            const double tick_ms = 1.0 / (double)c->wall_khz;
            const bool same_epoch = (d[8] >> 32) == d[5];
            snprintf(c->err, 512, "batch run again (device status %d): look-back of tile %llu gave up on tile %lld after %llu polls / %.1f ms (lane %llu, epoch %llu): words %016llx %016llx %016llx; "
                     "stuck tile's trace: epoch %llu%s HW_ID %08llx (wave %llu simd %llu cu %llu sh %llu se %llu) XCC %llu, ticket %.3f ms before the give-up, own totals %s, prefix %s",
                     derr, d[0] ? d[0] - 1 : 0ull, (long long)d[1], d[6], (double)(d[12] - d[13]) * tick_ms, d[7], d[5], d[2], d[3], d[4],
                     d[8] >> 32, same_epoch ? "" : " (NOT this run's: it never took its ticket here)", d[8] & 0xFFFFFFFFull, d[8] & 15, (d[8] >> 4) & 3, (d[8] >> 8) & 15, (d[8] >> 12) & 1, (d[8] >> 13) & 7, d[11] >> 56,
                     (double)(d[12] - d[9]) * tick_ms, d[10] ? "published" : "NOT published", (d[11] & 0x00FFFFFFFFFFFFFFull) ? "published" : "NOT published");
            if (!c->env_scan_budget) fprintf(stderr, "[libdartgpu] %s\n", c->err);
        }
        else { snprintf(c->err, 512, "device-side scan did not complete (status %d)", derr); return DG_ERR_INTERNAL; }
        if (attempt == 5) { snprintf(c->err, 512, "buffer capacities did not converge (status %d)", derr); return DG_ERR_INTERNAL; }
        if (derr != DG_E_SCAN && derr != DG_E_SEEDQ) c->reruns_capacity++;
        c->attempt_no = attempt + 1;
        const int rc = enqueue_run(c);
        if (rc) return rc;
    }
    c->enqueued = false;
    for (int i = 0; i < c->n_t; i++) { float ms = 0; (void)hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]); c->tms[i] = ms; }
    static_assert(CTR_N <= CTR_STRIDE, "the work counters fill one stripe");
    for (int k = 0; k < CTR_N; k++) c->counters[k] = c->h_tail->ctr[k];
    if (c->seed_qf_used) {
        // k_seed_qf keeps no per-lane tallies of its own work (they cost registers and moves in its loop): what it executed follows from the
        // slots its trips served -- one Occ step (one block; two when the interval straddles blocks, not counted) per slot of a step trip, one
        // prefix-table entry per slot of a begin trip, one SA entry and one text window per slot of a locate trip (k_seed_heavy adds its own)
        c->counters[CTR_STEPS_ACT] += c->counters[CTR_SQ_LANES + SQ_STEP]; c->counters[CTR_BLOCKS_ACT] += c->counters[CTR_SQ_LANES + SQ_STEP];
        c->counters[CTR_KTAB] += c->counters[CTR_SQ_LANES + SQ_BEGIN]; c->counters[CTR_DIRECT] += c->counters[CTR_SQ_LANES + SQ_LOC] + c->counters[CTR_SQ_LANES + SQ_CMP];
    }
    const DSizes &sz = c->h_tail->sizes;
    c->counters[CTR_SEEDS] = sz.total_seeds;
    const int derr = c->h_tail->err;
    if (derr) { snprintf(c->err, 512, "device pool exhausted (%s)", derr == DG_E_CIGAR ? "cigar" : (derr == DG_E_SJ ? "splice junction" : "reseed jobs")); return DG_ERR_INTERNAL; }
    c->used[0] = sz.total_rep; c->used[1] = sz.total_cig; c->used[2] = sz.total_sj;
    c->packed_valid = c->want_compact; c->full_valid = c->want_full || !c->want_compact;
    if (used) { used[0] = c->used[0]; used[1] = c->used[1]; used[2] = c->used[2]; }
    return DG_OK;
}

extern "C" int dg_batch_run(dg_ctx *c, size_t used[3])
{
    if (!c) return DG_ERR_ARG;
    if (c->no_batch) { snprintf(c->err, 512, "dg_batch_run: the context holds no batch (its last upload was a DG_FQ_CHECK_ONLY)"); return DG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    c->inf.valid = false;
    c->used[0] = c->used[1] = c->used[2] = 0;
    memset(c->counters, 0, sizeof c->counters);
    if (used) used[0] = used[1] = used[2] = 0;
    c->n_t = 0;
    c->packed_valid = false; c->full_valid = false; c->batch_done = false; c->sj.batch_counted = false; c->gc.batch_counted = false; c->tx.batch_counted = false; c->sam.valid = false; c->bam.valid = false; c->bam.rec_valid = false; c->bam.rec_stored = false;
    if (c->n_reads == 0) { c->batch_done = true; return DG_OK; }
    c->attempt_no = 0;
    int rc = enqueue_run(c);
    if (rc) return rc;
    rc = finish_run(c, used);
    c->batch_done = rc == DG_OK;
    return rc;
}

static int enqueue_download(dg_ctx *c, dg_read_out *ro, dg_report_out *po, uint32_t *cig, dg_sj_out *so, const size_t caps[3])
{
    if (caps[0] < c->used[0] || caps[1] < c->used[1] || caps[2] < c->used[2]) {
        snprintf(c->err, 512, "output capacity too small: reports %zu of %zu, cigar ops %zu of %zu, junction tuples %zu of %zu", c->used[0], caps[0], c->used[1], caps[1], c->used[2], caps[2]);
        return DG_ERR_CAPACITY;
    }
    c->dl_on_copy_stream = false;
    if (c->env_copy_stream >= 1 && c->ev_dl && host_page_locked(ro)) {   // (as in dg_batch_download_compact)
        std::lock_guard<std::mutex> lk(g_copy_mu[c->device & 63]);
        hipStream_t cs = nullptr;
        HIPCHK(copy_stream(c->device, 0, &cs));
        if (c->n_reads && ro) HIPCHK(hipMemcpyAsync(ro, c->reads_out.p, (size_t)c->n_reads * sizeof(dg_read_out), hipMemcpyDeviceToHost, cs));
        if (c->used[0] && po) HIPCHK(hipMemcpyAsync(po, c->reports.p, c->used[0] * sizeof(dg_report_out), hipMemcpyDeviceToHost, cs));
        if (c->used[1] && cig) HIPCHK(hipMemcpyAsync(cig, c->cigfinal.p, c->used[1] * 4, hipMemcpyDeviceToHost, cs));
        if (c->used[2] && so) HIPCHK(hipMemcpyAsync(so, c->sjfinal.p, c->used[2] * sizeof(dg_sj_out), hipMemcpyDeviceToHost, cs));
        HIPCHK(hipEventRecord(c->env_blocking_sync ? c->ev_dl_block : c->ev_dl, cs));
        c->dl_on_copy_stream = true;
        return DG_OK;
    }
    if (c->n_reads && ro) HIPCHK(hipMemcpyAsync(ro, c->reads_out.p, (size_t)c->n_reads * sizeof(dg_read_out), hipMemcpyDeviceToHost, c->stream));
    if (c->used[0] && po) HIPCHK(hipMemcpyAsync(po, c->reports.p, c->used[0] * sizeof(dg_report_out), hipMemcpyDeviceToHost, c->stream));
    if (c->used[1] && cig) HIPCHK(hipMemcpyAsync(cig, c->cigfinal.p, c->used[1] * 4, hipMemcpyDeviceToHost, c->stream));
    if (c->used[2] && so) HIPCHK(hipMemcpyAsync(so, c->sjfinal.p, c->used[2] * sizeof(dg_sj_out), hipMemcpyDeviceToHost, c->stream));
    return DG_OK;
}
// waits for what enqueue_download enqueued
static hipError_t wait_download(dg_ctx *c)
{
    if (c->dl_on_copy_stream) { c->dl_on_copy_stream = false; return hipEventSynchronize(c->env_blocking_sync ? c->ev_dl_block : c->ev_dl); }
    return wait_stream(c);
}

extern "C" int dg_batch_download_compact(dg_ctx *c, dg_read_c *ro, dg_report_c *po, uint32_t *cig, dg_sj_out *so, const size_t caps[3], size_t *n_ops_out)
{
    if (!c || !caps) return DG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (n_ops_out) *n_ops_out = 0;
    if (caps[0] < c->used[0] || caps[2] < c->used[2]) {
        snprintf(c->err, 512, "output capacity too small: reports %zu of %zu, junction tuples %zu of %zu", c->used[0], caps[0], c->used[2], caps[2]);
        return DG_ERR_CAPACITY;
    }
    const size_t n = (size_t)c->n_reads, nr = c->used[0];
    if (n == 0) return DG_OK;
    if (!c->packed_valid) {                       // (dg_batch_run and dg_map_batch_compact write the compact records beside the full ones; dg_map_batch* do not)
        snprintf(c->err, 512, "dg_batch_download_compact: the last batch was mapped through dg_map_batch / dg_map_batch_packed, which write the full records only");
        return DG_ERR_ARG;
    }
    if (c->h_tail->sizes.pad[1]) { snprintf(c->err, 512, "a record field does not fit the compact types: use dg_batch_download"); return DG_ERR_RANGE; }
    const size_t n_ops = (size_t)c->h_tail->sizes.pad[0];
    if (n_ops_out) *n_ops_out = n_ops;
    if (caps[1] < n_ops) { snprintf(c->err, 512, "output capacity too small: cigar ops %zu of %zu", n_ops, caps[1]); return DG_ERR_CAPACITY; }
    if (c->env_copy_stream >= 1 && c->ev_dl && host_page_locked(ro)) {
        {
            std::lock_guard<std::mutex> lk(g_copy_mu[c->device & 63]);        // (a context's copies and its event stay together in the shared stream)
            hipStream_t cs = nullptr;
            HIPCHK(copy_stream(c->device, 0, &cs));
            if (ro) HIPCHK(hipMemcpyAsync(ro, c->reads_c.p, n * sizeof(dg_read_c), hipMemcpyDeviceToHost, cs));
            if (nr && po) HIPCHK(hipMemcpyAsync(po, c->reports_c.p, nr * sizeof(dg_report_c), hipMemcpyDeviceToHost, cs));
            if (n_ops && cig) HIPCHK(hipMemcpyAsync(cig, c->cig_c.p, n_ops * 4, hipMemcpyDeviceToHost, cs));
            if (c->used[2] && so) HIPCHK(hipMemcpyAsync(so, c->sjfinal.p, c->used[2] * sizeof(dg_sj_out), hipMemcpyDeviceToHost, cs));
            HIPCHK(hipEventRecord(c->env_blocking_sync ? c->ev_dl_block : c->ev_dl, cs));
        }
        HIPCHK(hipEventSynchronize(c->env_blocking_sync ? c->ev_dl_block : c->ev_dl));
        return DG_OK;
    }
    if (ro) HIPCHK(hipMemcpyAsync(ro, c->reads_c.p, n * sizeof(dg_read_c), hipMemcpyDeviceToHost, c->stream));
    if (nr && po) HIPCHK(hipMemcpyAsync(po, c->reports_c.p, nr * sizeof(dg_report_c), hipMemcpyDeviceToHost, c->stream));
    if (n_ops && cig) HIPCHK(hipMemcpyAsync(cig, c->cig_c.p, n_ops * 4, hipMemcpyDeviceToHost, c->stream));
    if (c->used[2] && so) HIPCHK(hipMemcpyAsync(so, c->sjfinal.p, c->used[2] * sizeof(dg_sj_out), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));
    return DG_OK;
}

extern "C" int dg_map_batch_compact(dg_ctx *c, int n_reads, const uint32_t *seq_off, const uint16_t *rlen, const char *seq,
                                    int rlen_all, int words_per_read, const uint32_t *words, const uint32_t *nlist, size_t n_n,
                                    dg_read_c *ro, dg_report_c *po, uint32_t *cig, dg_sj_out *so, const size_t caps[3], size_t used[3])
{
    if (!c || !caps) return DG_ERR_ARG;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = words ? enqueue_upload_packed(c, n_reads, rlen_all, rlen, words_per_read, words, nlist, n_n) : enqueue_upload(c, n_reads, seq_off, rlen, seq);
    if (rc) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    c->want_full = false;                                   // this caller takes the compact records: the units k_pair finishes get no full ones (dg_batch_download would map the batch again)
    rc = dg_batch_run(c, used);
    c->want_full = true;
    if (rc) return rc;
    const auto t2 = std::chrono::steady_clock::now();
    size_t n_ops = 0;
    rc = dg_batch_download_compact(c, ro, po, cig, so, caps, &n_ops);
    const auto t3 = std::chrono::steady_clock::now();
    g_phase_ns[0] += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
    g_phase_ns[1] += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(t2 - t1).count();
    g_phase_ns[2] += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(t3 - t2).count();
    g_phase_ns[3] += 1;
    if (getenv("DG_HOST_PHASES") && (g_phase_ns[3] % 100) == 0)
        fprintf(stderr, "[dg host phases] batches %llu: upload enqueue %.3f ms, run (enqueue + wait) %.3f ms, download %.3f ms per batch\n", (unsigned long long)g_phase_ns[3],
                g_phase_ns[0] / 1e6 / g_phase_ns[3], g_phase_ns[1] / 1e6 / g_phase_ns[3], g_phase_ns[2] / 1e6 / g_phase_ns[3]);
    if (used && (rc == DG_OK || rc == DG_ERR_CAPACITY)) used[1] = n_ops ? n_ops : (rc == DG_OK ? 0 : used[1]);
    return rc;
}

// The full record types of the units k_pair finished are not written when the caller asked for the compact records only (dg_map_batch_compact): a caller that
// wants them after all (the compact types could not hold a field: DG_ERR_RANGE) gets the batch mapped again, with them -- the uploaded batch is still in HBM.
static int ensure_full_records(dg_ctx *c)
{
    if (c->full_valid || c->n_reads == 0) return DG_OK;
    const bool keep = c->want_full, counted = c->sj.batch_counted, stored = c->bam.rec_stored, genes = c->gc.batch_counted, txs = c->tx.batch_counted;
    c->want_full = true;
    size_t used[3];
    const int rc = dg_batch_run(c, used);
    c->want_full = keep;
    c->sj.batch_counted = counted;      // (the same batch, mapped again: its tuples are in the junction table already if they were before)
    c->bam.rec_stored = stored;         // (and its BAM records in the sorted store)
    c->gc.batch_counted = genes;        // (and its units in the gene table)
    c->tx.batch_counted = txs;          // (and in the class table)
    return rc;
}

extern "C" int dg_batch_download(dg_ctx *c, dg_read_out *ro, dg_report_out *po, uint32_t *cig, dg_sj_out *so, const size_t caps[3])
{
    if (!c || !caps) return DG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    { const int rf = ensure_full_records(c); if (rf) return rf; }
    const int rc = enqueue_download(c, ro, po, cig, so, caps);
    if (rc) return rc;
    HIPCHK(wait_download(c));
    return DG_OK;
}

// host buffers in, host records out: the copies and the kernels are enqueued back to back (two waits per batch: sizes, then
// records).  With page-locked caller buffers (dg_host_alloc) the copies are DMA transfers that overlap other contexts' kernels.
extern "C" int dg_map_batch(dg_ctx *c, int n_reads, const uint32_t *seq_off, const uint16_t *rlen, const char *seq,
                            dg_read_out *ro, dg_report_out *po, uint32_t *cig, dg_sj_out *so, const size_t caps[3], size_t used[3])
{
    if (!c || !caps) return DG_ERR_ARG;
    int rc = enqueue_upload(c, n_reads, seq_off, rlen, seq);
    if (rc) return rc;
    c->want_compact = false;                                // this caller takes the full records
    rc = dg_batch_run(c, used);
    c->want_compact = true;
    if (rc) return rc;
    return dg_batch_download(c, ro, po, cig, so, caps);
}

extern "C" int dg_map_batch_packed(dg_ctx *c, int n_reads, int rlen_all, const uint16_t *rlen, int words_per_read, const uint32_t *words,
                                   const uint32_t *nlist, size_t n_n, dg_read_out *ro, dg_report_out *po, uint32_t *cig, dg_sj_out *so,
                                   const size_t caps[3], size_t used[3])
{
    if (!c || !caps) return DG_ERR_ARG;
    int rc = enqueue_upload_packed(c, n_reads, rlen_all, rlen, words_per_read, words, nlist, n_n);
    if (rc) return rc;
    c->want_compact = false;
    rc = dg_batch_run(c, used);
    c->want_compact = true;
    if (rc) return rc;
    return dg_batch_download(c, ro, po, cig, so, caps);
}

extern "C" int dg_batch_device_ptrs(dg_ctx *c, void *ptrs[4])
{
    if (!c || !ptrs) return DG_ERR_ARG;
    { const int rf = ensure_full_records(c); if (rf) return rf; }
    ptrs[0] = c->reads_out.p; ptrs[1] = c->reports.p; ptrs[2] = c->cigfinal.p; ptrs[3] = c->sjfinal.p;
    return DG_OK;
}

extern "C" int dg_batch_device_ptrs_compact(dg_ctx *c, void *ptrs[2])
{
    if (!c || !ptrs) return DG_ERR_ARG;
    ptrs[0] = c->reads_c.p; ptrs[1] = c->reports_c.p;
    return DG_OK;
}

extern "C" int dg_batch_device_records_compact(dg_ctx *c, void *ptrs[4], size_t counts[4])
{
    if (!c || !ptrs || !counts) return DG_ERR_ARG;
    if (!c->packed_valid) { snprintf(c->err, 512, "dg_batch_device_records_compact: the last batch has no compact records (use dg_map_batch_compact / dg_batch_download_compact)"); return DG_ERR_ARG; }
    ptrs[0] = c->reads_c.p; ptrs[1] = c->reports_c.p; ptrs[2] = c->cig_c.p; ptrs[3] = c->sjfinal.p;
    counts[0] = (size_t)c->n_reads; counts[1] = c->used[0]; counts[2] = (size_t)c->h_tail->sizes.pad[0]; counts[3] = c->used[2];
    return DG_OK;
}

// ------------------------------------------------------------------------------------------
// SAM text on the device (dg_samfmt.h): the records of the batch that ran last -> the bytes the reference prints for them
// ------------------------------------------------------------------------------------------
extern "C" int dg_set_chr_names(dg_ctx *c, int n_chr, const uint32_t *name_off, const char *names)
{
    if (!c) return DG_ERR_ARG;
    IndexShared *sh = c->shared_ix;
    if (!sh || !name_off || n_chr != c->ix.n_chr) { snprintf(c->err, 512, "dg_set_chr_names: %d names for an index of %d chromosomes", n_chr, c->ix.n_chr); return DG_ERR_ARG; }
    for (int i = 0; i < n_chr; i++) if (name_off[i + 1] < name_off[i]) { snprintf(c->err, 512, "dg_set_chr_names: name_off decreases at %d", i); return DG_ERR_ARG; }
    if (name_off[n_chr] > name_off[0] && !names) { snprintf(c->err, 512, "dg_set_chr_names: names is NULL"); return DG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(sh->mu);
    std::vector<uint32_t> off((size_t)n_chr + 1);
    for (int i = 0; i <= n_chr; i++) off[i] = name_off[i] - name_off[0];
    uint32_t *d_off = nullptr; char *d_names = nullptr;
    HIPCHK(hipMalloc((void **)&d_off, off.size() * 4));
    if (hipMalloc((void **)&d_names, (size_t)off[n_chr] + 1) != hipSuccess) { (void)hipFree(d_off); return fail(c, DG_ERR_HIP, "hipMalloc (chromosome names)", hipErrorOutOfMemory); }
    hipError_t e = hipMemcpy(d_off, off.data(), off.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && off[n_chr]) e = hipMemcpy(d_names, names + name_off[0], off[n_chr], hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d_off); (void)hipFree(d_names); return fail(c, DG_ERR_HIP, "hipMemcpy (chromosome names)", e); }
    // A formatter of any context of this index reads the two pointers and enqueues its kernels under sh->mu (dg_batch_format_sam), so under the
    // lock every kernel that may read the old arrays is already in a stream: the device is waited for, then they are freed.
    if (sh->d_chr_name_off) { (void)hipDeviceSynchronize(); (void)hipFree(sh->d_chr_name_off); (void)hipFree(sh->d_chr_names); }
    sh->d_chr_name_off = d_off; sh->d_chr_names = d_names; sh->chr_names_set = true; sh->chr_names_gen++;
    sh->chr_name_max = 0;
    for (int i = 0; i < n_chr; i++) sh->chr_name_max = std::max(sh->chr_name_max, off[i + 1] - off[i]);
    return DG_OK;
}

static int sam_offsets_ok(dg_ctx *c, const char *what, const uint32_t *off, int n, const char *fn = "dg_batch_format_sam")
{
    for (int i = 0; i < n; i++) if (off[i + 1] < off[i]) { snprintf(c->err, 512, "%s: %s decreases at read %d", fn, what, i); return DG_ERR_ARG; }
    return DG_OK;
}

// what the entry points of both formatters check before they look at names and qualities (fn: the caller's name for the text; bam: the result that is reset)
static int sam_batch_ready(dg_ctx *c, int n_pair_mode, size_t *n_bytes, uint64_t counters[3], float *device_ms, const char *fn = "dg_batch_format_sam", bool bam = false)
{
    if (n_bytes) *n_bytes = 0;
    if (counters) counters[0] = counters[1] = counters[2] = 0;
    if (device_ms) *device_ms = 0.f;
    if (bam) { c->bam.valid = false; c->bam.bytes = 0; } else { c->sam.valid = false; c->sam.bytes = 0; }
    c->bam.rec_valid = false;           // (both formatters write the per-read offsets dg_batch_accumulate_bam walks)
    if (!c->batch_done) { snprintf(c->err, 512, "%s: the context has no finished batch (upload and run one first)", fn); return DG_ERR_ARG; }
    const int n = c->n_reads;
    if (n_pair_mode < 0 || (n_pair_mode & 1) || n_pair_mode > n) { snprintf(c->err, 512, "%s: n_pair_mode %d must be even and at most the batch's %d reads", fn, n_pair_mode, n); return DG_ERR_ARG; }
    if (n == 0) return DG_OK;
    if (c->enc_ready) { snprintf(c->err, 512, "%s: the batch was uploaded packed, and the pipeline keeps no ASCII copy of a packed batch: upload it as ASCII", fn); return DG_ERR_ARG; }
    if (!c->full_valid) { snprintf(c->err, 512, "%s: the last batch has no full records (it was mapped through dg_map_batch_compact)", fn); return DG_ERR_ARG; }
    IndexShared *sh = c->shared_ix;
    if (!sh || !sh->chr_names_set) { snprintf(c->err, 512, "%s: the chromosome names are missing (dg_set_chr_names)", fn); return DG_ERR_ARG; }
    return DG_OK;
}

// The formatter behind its inputs: names and qualities are in HBM (hdr / qual already moved back by their first offset; qual == nullptr: FASTA), whoever put
// them there -- dg_batch_format_sam's copies of the caller's arrays, enqueued just before, or the FASTQ upload.  Both entry points run these launches.
static int sam_format_device(dg_ctx *c, const uint32_t *hdr_off, const char *hdr, const uint32_t *qual_off, const char *qual, size_t hdr_bytes, size_t qual_bytes,
                             int n_pair_mode, uint32_t flags, size_t *n_bytes, uint64_t counters[3], float *device_ms)
{
    const int n = c->n_reads;
    IndexShared *sh = c->shared_ix;
    HIPCHK(c->sam.ready());
    const uint32_t n_tiles = (uint32_t)((n + SAM_LEN_THREADS - 1) / SAM_LEN_THREADS);
    HIPCHK(c->sam.qlen.ensure((size_t)n)); HIPCHK(c->sam.read_off.ensure((size_t)n)); HIPCHK(c->sam.tile.ensure(n_tiles));
    // the text's capacity is a guess the first time (one line per read); when it was too small k_sam_write alone runs again -- never the batch
    size_t want = hdr_bytes + qual_bytes + c->seq_bytes + (size_t)n * 96;
    want += want / 8;
    if (c->sam.first_cap && !c->sam.text.p) want = c->sam.first_cap;
    if (c->sam.text.cap < want) HIPCHK(c->sam.text.ensure(want));
    SamBatch b;
    b.ro = c->reads_out.p; b.po = c->reports.p; b.cig = c->cigfinal.p;
    b.seq_off = c->seq_off.p; b.rlen = c->rlen.p; b.seq = c->seq.p;
    b.hdr_off = hdr_off; b.hdr = hdr;
    b.qual_off = qual ? qual_off : nullptr; b.qual = qual;
    b.chr_off = nullptr; b.chr = nullptr; b.qlen = nullptr;      // (the names: under the index's lock, below)
    b.n_reads = n; b.n_pair_mode = n_pair_mode; b.unique_only = (flags & DG_SAM_UNIQUE_ONLY) ? 1 : 0; b.multi = c->pr.multi_hit ? 1 : 0;
    SamBatch b2 = b; uint64_t names_gen = 0;
    const unsigned grid = (unsigned)n;
    {   // the chromosome names are read and the kernels that use them enqueued under the index's lock: dg_set_chr_names, which replaces the
        // arrays under the same lock, waits for the device before it frees the old ones
        std::lock_guard<std::mutex> lk(sh->mu);
        b.chr_off = sh->d_chr_name_off; b.chr = sh->d_chr_names; names_gen = sh->chr_names_gen;
        b2 = b; b2.qlen = c->sam.qlen.p;
        HIPCHK(hipEventRecord(c->sam.ev[0], c->stream));
        HIPCHK(hipMemsetAsync(c->sam.stat.d, 0, 4 * 8, c->stream));
        k_sam_len<<<n_tiles, SAM_LEN_THREADS, 0, c->stream>>>(b, c->sam.read_off.p, c->sam.qlen.p, c->sam.tile.p, c->sam.stat.d);
        k_tiles_top<uint64_t><<<1, 256, 0, c->stream>>>(c->sam.tile.p, n_tiles, (uint64_t *)c->sam.stat.d);
        k_sam_write<<<grid, 64, 0, c->stream>>>(b2, c->sam.read_off.p, c->sam.tile.p, c->sam.stat.d, (unsigned long long)c->sam.text.cap, c->sam.text.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->sam.ev[1], c->stream));
    }
    HIPCHK(c->sam.stat.fetch(c->stream));
    HIPCHK(wait_stream(c));                                       // the one wait: for the size
    float ms = c->sam.ev.ms(0, 1);
    const size_t total = (size_t)c->sam.stat.h[0];
    if (total > c->sam.text.cap) {                                // the guess was too small (many lines per read): the lengths stand, the writer runs again
        HIPCHK(c->sam.text.ensure(total));
        {
            std::lock_guard<std::mutex> lk(sh->mu);
            if (names_gen != sh->chr_names_gen) { snprintf(c->err, 512, "dg_batch_format_sam: the chromosome names were replaced while the text was being formatted"); return DG_ERR_ARG; }
            HIPCHK(hipEventRecord(c->sam.ev[0], c->stream));
            k_sam_write<<<grid, 64, 0, c->stream>>>(b2, c->sam.read_off.p, c->sam.tile.p, c->sam.stat.d, (unsigned long long)c->sam.text.cap, c->sam.text.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(c->sam.ev[1], c->stream));
        }
        HIPCHK(wait_stream(c));
        ms += c->sam.ev.ms(0, 1);
    }
    c->sam.bytes = total; c->sam.valid = true;
    if (n_bytes) *n_bytes = total;
    if (counters) { counters[0] = c->sam.stat.h[1]; counters[1] = c->sam.stat.h[2]; counters[2] = c->sam.stat.h[3]; }
    if (device_ms) *device_ms = ms;
    return DG_OK;
}

extern "C" int dg_batch_format_sam(dg_ctx *c, const dg_sam_text *in, uint32_t flags, size_t *n_bytes, uint64_t counters[3], float *device_ms)
{
    if (!c) return DG_ERR_ARG;
    if (!in) {
        if (n_bytes) *n_bytes = 0;
        if (counters) counters[0] = counters[1] = counters[2] = 0;
        if (device_ms) *device_ms = 0.f;
        c->sam.valid = false; c->sam.bytes = 0;
        snprintf(c->err, 512, "dg_batch_format_sam: the input is NULL"); return DG_ERR_ARG;
    }
    const int rc = sam_batch_ready(c, in->n_pair_mode, n_bytes, counters, device_ms);
    if (rc) return rc;
    const int n = c->n_reads;
    if (n == 0) { c->sam.valid = true; return DG_OK; }
    if (!in->hdr_off || (in->qual && !in->qual_off)) { snprintf(c->err, 512, "dg_batch_format_sam: an offset array is NULL"); return DG_ERR_ARG; }
    if (sam_offsets_ok(c, "hdr_off", in->hdr_off, n) || (in->qual && sam_offsets_ok(c, "qual_off", in->qual_off, n))) return DG_ERR_ARG;
    const size_t hdr_bytes = (size_t)in->hdr_off[n] - in->hdr_off[0], qual_bytes = in->qual ? (size_t)in->qual_off[n] - in->qual_off[0] : 0;
    if (hdr_bytes && !in->hdr) { snprintf(c->err, 512, "dg_batch_format_sam: hdr is NULL"); return DG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->sam.hdr_off.ensure((size_t)n + 1)); HIPCHK(c->sam.hdr.ensure(hdr_bytes + 1));
    if (in->qual) { HIPCHK(c->sam.qual_off.ensure((size_t)n + 1)); HIPCHK(c->sam.qual.ensure(qual_bytes + 1)); }
    // offsets are taken relative to their first entry on the device: the kernels add them to pointers moved back by it
    HIPCHK(hipMemcpyAsync(c->sam.hdr_off.p, in->hdr_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, c->stream));
    if (hdr_bytes) HIPCHK(hipMemcpyAsync(c->sam.hdr.p, in->hdr + in->hdr_off[0], hdr_bytes, hipMemcpyHostToDevice, c->stream));
    if (in->qual) {
        HIPCHK(hipMemcpyAsync(c->sam.qual_off.p, in->qual_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, c->stream));
        if (qual_bytes) HIPCHK(hipMemcpyAsync(c->sam.qual.p, in->qual + in->qual_off[0], qual_bytes, hipMemcpyHostToDevice, c->stream));
    }
    return sam_format_device(c, c->sam.hdr_off.p, c->sam.hdr.p - in->hdr_off[0], in->qual ? c->sam.qual_off.p : nullptr, in->qual ? c->sam.qual.p - in->qual_off[0] : nullptr,
                             hdr_bytes, qual_bytes, in->n_pair_mode, flags, n_bytes, counters, device_ms);
}

extern "C" int dg_batch_format_sam_resident(dg_ctx *c, int n_pair_mode, uint32_t flags, size_t *n_bytes, uint64_t counters[3], float *device_ms)
{
    if (!c) return DG_ERR_ARG;
    const int rc = sam_batch_ready(c, n_pair_mode, n_bytes, counters, device_ms);
    if (rc) return rc;
    if (!c->fq.valid) { snprintf(c->err, 512, "dg_batch_format_sam_resident: the context's last upload was not dg_batch_upload_fastq: no names and qualities in HBM"); return DG_ERR_ARG; }
    if (c->n_reads == 0) { c->sam.valid = true; return DG_OK; }
    HIPCHK(hipSetDevice(c->device));
    return sam_format_device(c, c->fq.hdr_off.p, c->fq.hdr.p, c->fq.qual_off.p, c->fq.qual.p, c->fq.hdr_bytes, c->fq.qual_bytes, n_pair_mode, flags, n_bytes, counters, device_ms);
}

extern "C" int dg_batch_download_sam(dg_ctx *c, char *out, size_t cap)
{
    if (!c) return DG_ERR_ARG;
    if (!c->sam.valid) { snprintf(c->err, 512, "dg_batch_download_sam: no SAM text (dg_batch_format_sam first)"); return DG_ERR_ARG; }
    if (cap < c->sam.bytes) { snprintf(c->err, 512, "dg_batch_download_sam: output capacity too small: %zu bytes of %zu", cap, c->sam.bytes); return DG_ERR_CAPACITY; }
    if (c->sam.bytes == 0) return DG_OK;
    if (!out) return DG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(out, c->sam.text.p, c->sam.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));
    return DG_OK;
}

extern "C" int dg_batch_device_sam(dg_ctx *c, void **ptr, size_t *n_bytes)
{
    if (!c || !ptr || !n_bytes) return DG_ERR_ARG;
    if (!c->sam.valid) { snprintf(c->err, 512, "dg_batch_device_sam: no SAM text (dg_batch_format_sam first)"); return DG_ERR_ARG; }
    *ptr = c->sam.bytes ? c->sam.text.p : nullptr; *n_bytes = c->sam.bytes;
    return DG_OK;
}

// ------------------------------------------------------------------------------------------
// BAM on the device (dg_bamfmt.h, dg_bgzf.h): the records of the batch that ran last -> uncompressed BAM records -> BGZF blocks
// ------------------------------------------------------------------------------------------
// n bytes in HBM (4-byte aligned, readable up to the next multiple of 4) -> BGZF blocks in c->bam.bgzf_out: three launches and one wait, for the size;
// dynamic: Huffman codes per strip (k_bgzf_deflate_dyn) in place of the fixed code
static int bgzf_device(dg_ctx *c, const unsigned char *d_in, size_t n, bool dynamic, size_t *n_out, float *ms, unsigned long long *d_phases = nullptr)
{
    *n_out = 0; *ms = 0.f;
    const size_t blocks = (n + BGZF_BLOCK - 1) / BGZF_BLOCK;
    if (!blocks) return DG_OK;
    if (blocks > 0x7fffffffull) { snprintf(c->err, 512, "BGZF: %zu bytes are more than one call takes", n); return DG_ERR_ARG; }
    HIPCHK(c->bam.bgzf_slots.ensure(blocks * BGZF_SLOT)); HIPCHK(c->bam.bgzf_size.ensure(blocks)); HIPCHK(c->bam.bgzf_off.ensure(blocks));
    HIPCHK(c->bam.bgzf_out.ensure(n + (size_t)BGZF_OVERHEAD * blocks));                 // the bound of the stored form: no block is larger
    HIPCHK(hipEventRecord(c->bam.ev[0], c->stream));
    if (dynamic) k_bgzf_deflate_dyn<<<(unsigned)blocks, BGZF_THREADS, 0, c->stream>>>(d_in, (unsigned long long)n, c->bam.bgzf_slots.p, c->bam.bgzf_off.p, c->bam.bgzf_size.p, d_phases);
    else k_bgzf_deflate<<<(unsigned)blocks, BGZF_THREADS, 0, c->stream>>>(d_in, (unsigned long long)n, c->bam.bgzf_slots.p, c->bam.bgzf_off.p, c->bam.bgzf_size.p);
    k_tiles_top<uint64_t><<<1, 256, 0, c->stream>>>(c->bam.bgzf_off.p, (uint32_t)blocks, (uint64_t *)(c->bam.stat.d + 6));
    k_bgzf_copy<<<(unsigned)blocks, 256, 0, c->stream>>>(c->bam.bgzf_slots.p, c->bam.bgzf_off.p, c->bam.bgzf_size.p, c->bam.bgzf_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->bam.ev[1], c->stream));
    HIPCHK(hipMemcpyAsync(c->bam.stat.h + 6, c->bam.stat.d + 6, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));
    *ms = c->bam.ev.ms(0, 1);
    *n_out = (size_t)c->bam.stat.h[6];
    if (*n_out > n + (size_t)BGZF_OVERHEAD * blocks) { snprintf(c->err, 512, "BGZF: %zu bytes of blocks for %zu bytes", *n_out, n); return DG_ERR_INTERNAL; }
    return DG_OK;
}

// The writer behind its inputs, as sam_format_device: names and qualities are in HBM.  Both entry points run these launches.
static int bam_format_device(dg_ctx *c, const uint32_t *hdr_off, const char *hdr, const uint32_t *qual_off, const char *qual, size_t hdr_bytes, size_t qual_bytes,
                             int n_pair_mode, uint32_t flags, size_t *n_bytes, size_t *n_raw, uint64_t counters[5], float *device_ms)
{
    const int n = c->n_reads;
    IndexShared *sh = c->shared_ix;
    HIPCHK(c->bam.ready());
    const uint32_t n_tiles = (uint32_t)((n + SAM_LEN_THREADS - 1) / SAM_LEN_THREADS);
    HIPCHK(c->sam.qlen.ensure((size_t)n)); HIPCHK(c->sam.read_off.ensure((size_t)n)); HIPCHK(c->sam.tile.ensure(n_tiles));
    // the capacity is a guess the first time (one record per read); when it was too small k_bam_write alone runs again -- never the batch
    size_t want = hdr_bytes + qual_bytes + c->seq_bytes / 2 + (size_t)n * 64;
    want += want / 8;
    if (c->bam.first_cap && !c->bam.rec.p) want = c->bam.first_cap;
    if (c->bam.rec.cap < want + 8) HIPCHK(c->bam.rec.ensure(want + 8));
    SamBatch b;
    b.ro = c->reads_out.p; b.po = c->reports.p; b.cig = c->cigfinal.p;
    b.seq_off = c->seq_off.p; b.rlen = c->rlen.p; b.seq = c->seq.p;
    b.hdr_off = hdr_off; b.hdr = hdr;
    b.qual_off = qual ? qual_off : nullptr; b.qual = qual;
    b.chr_off = nullptr; b.chr = nullptr; b.qlen = nullptr;
    b.n_reads = n; b.n_pair_mode = n_pair_mode; b.unique_only = (flags & DG_SAM_UNIQUE_ONLY) ? 1 : 0; b.multi = c->pr.multi_hit ? 1 : 0;
    SamBatch b2 = b;
    const unsigned grid = (unsigned)n;
    {   // k_bam_len takes its counters from the SAM formatter's length pass, which reads the chromosome names: enqueued under the index's lock, as there
        std::lock_guard<std::mutex> lk(sh->mu);
        b.chr_off = sh->d_chr_name_off; b.chr = sh->d_chr_names;
        b2.qlen = c->sam.qlen.p;                                  // (the writer reads no names)
        HIPCHK(hipEventRecord(c->bam.ev[0], c->stream));
        HIPCHK(hipMemsetAsync(c->bam.stat.d, 0, 8 * 8, c->stream));
        k_bam_len<<<n_tiles, SAM_LEN_THREADS, 0, c->stream>>>(b, c->sam.read_off.p, c->sam.qlen.p, c->sam.tile.p, c->bam.stat.d);
        k_tiles_top<uint64_t><<<1, 256, 0, c->stream>>>(c->sam.tile.p, n_tiles, (uint64_t *)c->bam.stat.d);
        k_bam_write<<<grid, 64, 0, c->stream>>>(b2, c->sam.read_off.p, c->sam.tile.p, c->bam.stat.d, (unsigned long long)(c->bam.rec.cap - 8), c->bam.rec.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->bam.ev[1], c->stream));
    }
    HIPCHK(hipMemcpyAsync(c->bam.stat.h, c->bam.stat.d, 6 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));                                       // the first wait: for the records' size
    float ms = c->bam.ev.ms(0, 1);
    const size_t total = (size_t)c->bam.stat.h[0];
    if (total > c->bam.rec.cap - 8) {                             // the guess was too small: the lengths stand, the writer runs again
        HIPCHK(c->bam.rec.ensure(total + 8));
        HIPCHK(hipEventRecord(c->bam.ev[0], c->stream));
        k_bam_write<<<grid, 64, 0, c->stream>>>(b2, c->sam.read_off.p, c->sam.tile.p, c->bam.stat.d, (unsigned long long)(c->bam.rec.cap - 8), c->bam.rec.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->bam.ev[1], c->stream));
        HIPCHK(wait_stream(c));
        ms += c->bam.ev.ms(0, 1);
    }
    size_t out_bytes = total;
    c->bam.ptr = c->bam.rec.p;
    c->bam.ms[0] = ms; c->bam.ms[1] = 0.f;
    if (!(flags & DG_BAM_RAW) && total) {
        float ms_z = 0.f;
        const int rc = bgzf_device(c, c->bam.rec.p, total, (flags & DG_BAM_DYNAMIC) != 0, &out_bytes, &ms_z);      // the second wait: for the stream's size
        if (rc) return rc;
        ms += ms_z; c->bam.ms[1] = ms_z;
        c->bam.ptr = c->bam.bgzf_out.p;
    }
    c->bam.bytes = out_bytes; c->bam.valid = true;
    c->bam.rec_valid = true; c->bam.rec_bytes = total; c->bam.rec_records = (size_t)c->bam.stat.h[4];
    if (n_bytes) *n_bytes = out_bytes;
    if (n_raw) *n_raw = total;
    if (counters) for (int i = 0; i < 5; i++) counters[i] = c->bam.stat.h[1 + i];
    if (device_ms) *device_ms = ms;
    return DG_OK;
}

static void bam_outputs_zero(size_t *n_raw, uint64_t counters[5]) { if (n_raw) *n_raw = 0; if (counters) counters[3] = counters[4] = 0; }

extern "C" int dg_batch_format_bam(dg_ctx *c, const dg_sam_text *in, uint32_t flags, size_t *n_bytes, size_t *n_raw, uint64_t counters[5], float *device_ms)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_batch_format_bam";
    bam_outputs_zero(n_raw, counters);
    if (!in) {
        if (n_bytes) *n_bytes = 0;
        if (counters) counters[0] = counters[1] = counters[2] = 0;
        if (device_ms) *device_ms = 0.f;
        c->bam.valid = false; c->bam.bytes = 0;
        snprintf(c->err, 512, "%s: the input is NULL", fn); return DG_ERR_ARG;
    }
    const int rc = sam_batch_ready(c, in->n_pair_mode, n_bytes, counters, device_ms, fn, true);
    if (rc) return rc;
    const int n = c->n_reads;
    if (n == 0) { c->bam.valid = true; c->bam.ptr = nullptr; c->bam.rec_valid = true; c->bam.rec_bytes = c->bam.rec_records = 0; return DG_OK; }
    if (!in->hdr_off || (in->qual && !in->qual_off)) { snprintf(c->err, 512, "%s: an offset array is NULL", fn); return DG_ERR_ARG; }
    if (sam_offsets_ok(c, "hdr_off", in->hdr_off, n, fn) || (in->qual && sam_offsets_ok(c, "qual_off", in->qual_off, n, fn))) return DG_ERR_ARG;
    const size_t hdr_bytes = (size_t)in->hdr_off[n] - in->hdr_off[0], qual_bytes = in->qual ? (size_t)in->qual_off[n] - in->qual_off[0] : 0;
    if (hdr_bytes && !in->hdr) { snprintf(c->err, 512, "%s: hdr is NULL", fn); return DG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->sam.hdr_off.ensure((size_t)n + 1)); HIPCHK(c->sam.hdr.ensure(hdr_bytes + 1));
    if (in->qual) { HIPCHK(c->sam.qual_off.ensure((size_t)n + 1)); HIPCHK(c->sam.qual.ensure(qual_bytes + 1)); }
    HIPCHK(hipMemcpyAsync(c->sam.hdr_off.p, in->hdr_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, c->stream));
    if (hdr_bytes) HIPCHK(hipMemcpyAsync(c->sam.hdr.p, in->hdr + in->hdr_off[0], hdr_bytes, hipMemcpyHostToDevice, c->stream));
    if (in->qual) {
        HIPCHK(hipMemcpyAsync(c->sam.qual_off.p, in->qual_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, c->stream));
        if (qual_bytes) HIPCHK(hipMemcpyAsync(c->sam.qual.p, in->qual + in->qual_off[0], qual_bytes, hipMemcpyHostToDevice, c->stream));
    }
    return bam_format_device(c, c->sam.hdr_off.p, c->sam.hdr.p - in->hdr_off[0], in->qual ? c->sam.qual_off.p : nullptr, in->qual ? c->sam.qual.p - in->qual_off[0] : nullptr,
                             hdr_bytes, qual_bytes, in->n_pair_mode, flags, n_bytes, n_raw, counters, device_ms);
}

extern "C" int dg_batch_format_bam_resident(dg_ctx *c, int n_pair_mode, uint32_t flags, size_t *n_bytes, size_t *n_raw, uint64_t counters[5], float *device_ms)
{
    if (!c) return DG_ERR_ARG;
    bam_outputs_zero(n_raw, counters);
    const int rc = sam_batch_ready(c, n_pair_mode, n_bytes, counters, device_ms, "dg_batch_format_bam_resident", true);
    if (rc) return rc;
    if (!c->fq.valid) { snprintf(c->err, 512, "dg_batch_format_bam_resident: the context's last upload was not dg_batch_upload_fastq: no names and qualities in HBM"); return DG_ERR_ARG; }
    if (c->n_reads == 0) { c->bam.valid = true; c->bam.ptr = nullptr; c->bam.rec_valid = true; c->bam.rec_bytes = c->bam.rec_records = 0; return DG_OK; }
    HIPCHK(hipSetDevice(c->device));
    return bam_format_device(c, c->fq.hdr_off.p, c->fq.hdr.p, c->fq.qual_off.p, c->fq.qual.p, c->fq.hdr_bytes, c->fq.qual_bytes, n_pair_mode, flags, n_bytes, n_raw, counters, device_ms);
}

extern "C" int dg_batch_download_bam(dg_ctx *c, void *out, size_t cap)
{
    if (!c) return DG_ERR_ARG;
    if (!c->bam.valid) { snprintf(c->err, 512, "dg_batch_download_bam: no BAM bytes (dg_batch_format_bam or dg_bgzf_compress first)"); return DG_ERR_ARG; }
    if (cap < c->bam.bytes) { snprintf(c->err, 512, "dg_batch_download_bam: output capacity too small: %zu bytes of %zu", cap, c->bam.bytes); return DG_ERR_CAPACITY; }
    if (c->bam.bytes == 0) return DG_OK;
    if (!out) return DG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(out, c->bam.ptr, c->bam.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));
    return DG_OK;
}

extern "C" int dg_batch_device_bam(dg_ctx *c, void **ptr, size_t *n_bytes)
{
    if (!c || !ptr || !n_bytes) return DG_ERR_ARG;
    if (!c->bam.valid) { snprintf(c->err, 512, "dg_batch_device_bam: no BAM bytes (dg_batch_format_bam or dg_bgzf_compress first)"); return DG_ERR_ARG; }
    *ptr = c->bam.bytes ? c->bam.ptr : nullptr; *n_bytes = c->bam.bytes;
    return DG_OK;
}

extern "C" int dg_bgzf_compress_flags(dg_ctx *c, const void *host_bytes, size_t n, uint32_t flags, size_t *n_bytes, float *device_ms)
{
    if (!c) return DG_ERR_ARG;
    if (n_bytes) *n_bytes = 0;
    if (device_ms) *device_ms = 0.f;
    c->bam.valid = false; c->bam.bytes = 0; c->bam.ptr = nullptr;
    if (flags & ~DG_BGZF_DYNAMIC) { snprintf(c->err, 512, "dg_bgzf_compress_flags: unknown flag bits 0x%x", flags & ~DG_BGZF_DYNAMIC); return DG_ERR_ARG; }
    if (n == 0) { c->bam.valid = true; return DG_OK; }
    if (!host_bytes) { snprintf(c->err, 512, "dg_bgzf_compress: the input is NULL"); return DG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->bam.ready());
    HIPCHK(c->bam.bgzf_in.ensure(n + 8));
    HIPCHK(hipMemcpyAsync(c->bam.bgzf_in.p, host_bytes, n, hipMemcpyHostToDevice, c->stream));
    size_t out_bytes = 0; float ms = 0.f;
    const int rc = bgzf_device(c, c->bam.bgzf_in.p, n, (flags & DG_BGZF_DYNAMIC) != 0, &out_bytes, &ms);
    if (rc) return rc;
    c->bam.ptr = c->bam.bgzf_out.p; c->bam.bytes = out_bytes; c->bam.valid = true;
    c->bam.ms[0] = 0.f; c->bam.ms[1] = ms;
    if (n_bytes) *n_bytes = out_bytes;
    if (device_ms) *device_ms = ms;
    return DG_OK;
}

extern "C" int dg_bgzf_compress(dg_ctx *c, const void *host_bytes, size_t n, size_t *n_bytes, float *device_ms)
{
    return dg_bgzf_compress_flags(c, host_bytes, n, 0u, n_bytes, device_ms);
}

extern "C" int dg_batch_bam_device_ms(dg_ctx *c, float ms[2])
{
    if (!c || !ms) return DG_ERR_ARG;
    ms[0] = c->bam.ms[0]; ms[1] = c->bam.ms[1];
    return DG_OK;
}

extern "C" int dg_bgzf_granules(int out[2])
{
    if (!out) return DG_ERR_ARG;
    out[0] = (int)BGZF_STRIP; out[1] = (int)BGZF_SEG;
    return DG_OK;
}

// ------------------------------------------------------------------------------------------
// the splice-junction table on the device (dg_sjtab.h): count per batch, sort and print at the end of the job
// ------------------------------------------------------------------------------------------
static size_t sj_round_slots(size_t slots)
{
    size_t s = SJ_MIN_SLOTS;
    while (s < slots && s < ((size_t)1 << 40)) s <<= 1;
    return s;
}
// an empty table of `slots` (a power of two) in place of the context's; the old one is handed back through *old (the caller frees it) or freed here
static int sj_new_table(dg_ctx *c, size_t slots, SjSlot **old)
{
    SjSlot *t = nullptr;
    HIPCHK(hipMalloc((void **)&t, slots * sizeof(SjSlot)));
    const hipError_t e = hipMemsetAsync(t, 0, slots * sizeof(SjSlot), c->stream);
    if (e != hipSuccess) { (void)hipFree(t); return fail(c, DG_ERR_HIP, "hipMemsetAsync (junction table)", e); }
    if (old) *old = c->sj.tab;
    else if (c->sj.tab) { (void)hipStreamSynchronize(c->stream); (void)hipFree(c->sj.tab); }
    c->sj.tab = t; c->sj.slots = slots;
    return DG_OK;
}
static int sj_ready(dg_ctx *c)
{
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->sj.ready());
    c->sj.fin_valid = false;
    if (!c->sj.tab) return sj_new_table(c, SJ_FIRST_SLOTS, nullptr);
    return DG_OK;
}
static void sj_launch_insert(dg_ctx *c, const void *src, size_t n, int kind, DBuf<dg_sj_entry> &ovf)
{
    if (!n) return;
    k_sj_insert<<<(unsigned)((n + SJ_THREADS - 1) / SJ_THREADS), SJ_THREADS, 0, c->stream>>>((const unsigned char *)src, (unsigned long long)n, kind, c->sj.tab,
                                                                                          (unsigned long long)(c->sj.slots - 1), ovf.p, (unsigned long long)ovf.cap, c->sj.stat.d);
}
// Items in device memory (on this context's stream, or ordered before it) into the table: one insert pass, one wait; then, while an item found no slot or more
// than half the slots hold a key, a table of twice the size takes the old slots with their counts and ONLY the items of the overflow list, so every item is
// counted exactly once -- a pass is never run again whole.
static int sj_insert(dg_ctx *c, const void *src, size_t n, int kind)
{
    if (n >= 0xFFFFFF00ull * SJ_THREADS) { snprintf(c->err, 512, "junction table: too many items in one call"); return DG_ERR_ARG; }
    int cur = c->sj.ovf_cur;
    HIPCHK(c->sj.ovf[cur].ensure(n));                             // the overflow list: a bump pointer with room for every item of the pass
    HIPCHK(hipMemsetAsync(c->sj.stat.d + SJ_ST_OVERFLOW, 0, 8, c->stream));
    sj_launch_insert(c, src, n, kind, c->sj.ovf[cur]);
    HIPCHK(hipGetLastError());
    for (int round = 0; ; round++) {
        HIPCHK(hipMemcpyAsync(c->sj.stat.h, c->sj.stat.d, 3 * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(wait_stream(c));
        const size_t n_ovf = (size_t)c->sj.stat.h[SJ_ST_OVERFLOW];
        c->sj.distinct = (size_t)c->sj.stat.h[SJ_ST_DISTINCT];
        if (n_ovf > c->sj.ovf[cur].cap) { snprintf(c->err, 512, "junction table: the overflow list outgrew its capacity (%zu of %zu)", n_ovf, c->sj.ovf[cur].cap); return DG_ERR_INTERNAL; }
        if (n_ovf == 0 && c->sj.distinct <= c->sj.slots / 2) break;
        if (round >= 40 || c->sj.slots >= ((size_t)1 << 40)) { snprintf(c->err, 512, "junction table: growth did not converge at %zu slots", c->sj.slots); return DG_ERR_INTERNAL; }
        const int nxt = cur ^ 1;
        const size_t old_slots = c->sj.slots, old_keys = c->sj.distinct;
        HIPCHK(c->sj.ovf[nxt].ensure(old_keys + n_ovf));
        SjSlot *old = nullptr;
        { const int rc = sj_new_table(c, old_slots * 2, &old); if (rc) return rc; }
        hipError_t e = hipMemsetAsync(c->sj.stat.d, 0, 2 * 8, c->stream);        // the overflow and the distinct counts: the new table counts its keys itself
        if (e == hipSuccess) {
            sj_launch_insert(c, old, old_slots, SJ_SRC_SLOTS, c->sj.ovf[nxt]);
            sj_launch_insert(c, c->sj.ovf[cur].p, n_ovf, SJ_SRC_ENTRIES, c->sj.ovf[nxt]);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        (void)hipFree(old);
        if (e != hipSuccess) return fail(c, DG_ERR_HIP, "junction table growth", e);
        cur = nxt; c->sj.ovf_cur = cur;
    }
    return DG_OK;
}
// an insert pass may have met a coordinate the table cannot hold (INT64_MIN): said once the pass is over, the other items are counted
static int sj_refused(dg_ctx *c, const char *fn)
{
    const size_t bad = (size_t)c->sj.stat.h[SJ_ST_REFUSED];
    if (!bad) return DG_OK;
    (void)hipMemsetAsync(c->sj.stat.d + SJ_ST_REFUSED, 0, 8, c->stream);
    snprintf(c->err, 512, "%s: %zu tuples hold the coordinate INT64_MIN, which the table does not store; the others were counted", fn, bad);
    return DG_ERR_RANGE;
}

extern "C" int dg_sj_granules(int out[2])
{
    if (!out) return DG_ERR_ARG;
    out[0] = SJ_THREADS; out[1] = SJ_MIN_SLOTS;
    return DG_OK;
}

extern "C" int dg_sj_reserve(dg_ctx *c, size_t slots)
{
    if (!c) return DG_ERR_ARG;
    if (c->sj.distinct) { snprintf(c->err, 512, "dg_sj_reserve: the table holds %zu keys (dg_sj_reset first)", c->sj.distinct); return DG_ERR_ARG; }
    if (slots > ((size_t)1 << 36)) { snprintf(c->err, 512, "dg_sj_reserve: %zu slots are more than the table takes", slots); return DG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->sj.ready());
    c->sj.fin_valid = false;
    return sj_new_table(c, sj_round_slots(slots), nullptr);
}

extern "C" int dg_sj_reset(dg_ctx *c)
{
    if (!c) return DG_ERR_ARG;
    { const int rc = sj_ready(c); if (rc) return rc; }
    HIPCHK(hipMemsetAsync(c->sj.tab, 0, c->sj.slots * sizeof(SjSlot), c->stream));
    HIPCHK(hipMemsetAsync(c->sj.stat.d, 0, SJ_ST_WORDS * 8, c->stream));
    HIPCHK(wait_stream(c));
    c->sj.distinct = 0;
    return DG_OK;
}

extern "C" int dg_batch_accumulate_sj(dg_ctx *c, size_t *n_tuples)
{
    if (!c) return DG_ERR_ARG;
    if (n_tuples) *n_tuples = 0;
    if (!c->batch_done) { snprintf(c->err, 512, "dg_batch_accumulate_sj: the context has no finished batch (upload and run one first)"); return DG_ERR_ARG; }
    if (c->sj.batch_counted) { snprintf(c->err, 512, "dg_batch_accumulate_sj: the tuples of this batch are in the table already (a batch is counted once)"); return DG_ERR_ARG; }
    { const int rc = sj_ready(c); if (rc) return rc; }
    const size_t n = c->n_reads ? c->used[2] : 0;
    if (n) { const int rc = sj_insert(c, c->sjfinal.p, n, SJ_SRC_TUPLES); if (rc) return rc; }
    c->sj.batch_counted = true;
    if (n_tuples) *n_tuples = n;
    return n ? sj_refused(c, "dg_batch_accumulate_sj") : DG_OK;
}

extern "C" int dg_sj_add(dg_ctx *c, const dg_sj_entry *entries, size_t n)
{
    if (!c || (n && !entries)) return DG_ERR_ARG;
    for (size_t i = 0; i < n; i++)
        if (entries[i].count && !sj_key_ok(entries[i].g1, entries[i].g2)) { snprintf(c->err, 512, "dg_sj_add: entry %zu holds the coordinate INT64_MIN, which the table does not store", i); return DG_ERR_ARG; }
    { const int rc = sj_ready(c); if (rc) return rc; }
    if (!n) return DG_OK;
    HIPCHK(c->sj.in.ensure(n));
    HIPCHK(hipMemcpyAsync(c->sj.in.p, entries, n * sizeof(dg_sj_entry), hipMemcpyHostToDevice, c->stream));
    return sj_insert(c, c->sj.in.p, n, SJ_SRC_ENTRIES);
}

extern "C" int dg_sj_merge(dg_ctx *dst, dg_ctx *src)
{
    dg_ctx *c = dst;
    if (!dst || !src) return DG_ERR_ARG;
    if (dst == src || dst->device != src->device) { snprintf(c->err, 512, "dg_sj_merge: the two contexts must differ and be on one device"); return DG_ERR_ARG; }
    { const int rc = sj_ready(dst); if (rc) return rc; }
    src->sj.fin_valid = false;
    if (!src->sj.tab || !src->sj.distinct) return DG_OK;
    HIPCHK(src->sj.ready());
    // behind everything the source's stream holds; the source's table is emptied on the destination's stream, which the call waits for
    HIPCHK(hipEventRecord(src->sj.ev[2], src->stream));
    HIPCHK(hipStreamWaitEvent(dst->stream, src->sj.ev[2], 0));
    const int rc = sj_insert(dst, src->sj.tab, src->sj.slots, SJ_SRC_SLOTS);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(src->sj.tab, 0, src->sj.slots * sizeof(SjSlot), dst->stream));
    HIPCHK(hipMemsetAsync(src->sj.stat.d, 0, SJ_ST_WORDS * 8, dst->stream));
    HIPCHK(wait_stream(dst));
    src->sj.distinct = 0;
    return DG_OK;
}

// the scratch of a sort of n pairs: the one place that sizes it
inline hipError_t SortBufs::ensure(uint32_t n)
{
    hipError_t e = hist.ensure(rs_hist_words(n));
    if (e != hipSuccess) { short_of = "the sorter's histograms"; short_bytes = rs_hist_words(n) * sizeof(uint32_t); return e; }
    e = sums.ensure(rs_sums_words(n));
    if (e != hipSuccess) { short_of = "the sorter's sums"; short_bytes = rs_sums_words(n) * sizeof(uint32_t); }
    return e;
}
inline int SortBufs::sort(dg_ctx *c, uint32_t n, int bits, int &which)
{
    uint64_t *const keys[2] = {k[0].p, k[1].p}; int64_t *const vals[2] = {v[0].p, v[1].p};
    const hipError_t e = rs_sort_passes(c->stream, keys, vals, hist.p, sums.p, n, bits, which);
    return e == hipSuccess ? DG_OK : fail(c, DG_ERR_HIP, "hipGetLastError()", e);
}

extern "C" int dg_sj_finish(dg_ctx *c, uint32_t flags, size_t *n_entries, size_t *n_lines, size_t *n_bytes, float *device_ms)
{
    if (!c) return DG_ERR_ARG;
    if (n_entries) *n_entries = 0;
    if (n_lines) *n_lines = 0;
    if (n_bytes) *n_bytes = 0;
    if (device_ms) *device_ms = 0.f;
    const bool text = !(flags & DG_SJ_ENTRIES_ONLY);
    IndexShared *sh = c->shared_ix;
    c->sj.fin_valid = false;
    if (text && (!sh || !sh->chr_names_set)) { snprintf(c->err, 512, "dg_sj_finish: the chromosome names are missing (dg_set_chr_names), and DG_SJ_ENTRIES_ONLY is not set"); return DG_ERR_ARG; }
    { const int rc = sj_ready(c); if (rc) return rc; }
    c->sj.fin_entries = 0; c->sj.fin_bytes = 0;
    if (!c->sj.distinct) { c->sj.fin_valid = true; return DG_OK; }
    if (c->sj.distinct >= 0xFFFFF000ull) { snprintf(c->err, 512, "dg_sj_finish: %zu entries are more than the sorter takes", c->sj.distinct); return DG_ERR_ARG; }
    const size_t cap = c->sj.distinct;
    for (int k = 0; k < 2; k++) { HIPCHK(c->sj.sort.k[k].ensure(cap)); HIPCHK(c->sj.sort.v[k].ensure(cap)); }
    HIPCHK(c->sj.entries.ensure(cap)); HIPCHK(c->sj.line_off.ensure(cap));
    const uint32_t n_tiles = (uint32_t)((cap + SJ_THREADS - 1) / SJ_THREADS);
    HIPCHK(c->sj.tile.ensure(n_tiles));
    HIPCHK(hipEventRecord(c->sj.ev[0], c->stream));
    HIPCHK(hipMemsetAsync(c->sj.stat.d + SJ_ST_ENTRIES, 0, (SJ_ST_WORDS - SJ_ST_ENTRIES) * 8, c->stream));
    k_sj_compact<<<(unsigned)((c->sj.slots + SJ_THREADS - 1) / SJ_THREADS), SJ_THREADS, 0, c->stream>>>(c->sj.tab, (unsigned long long)c->sj.slots, (unsigned long long)cap, c->sj.sort.k[0].p, c->sj.sort.v[0].p, c->sj.stat.d);
    HIPCHK(hipGetLastError());
    HIPCHK(c->sj.stat.fetch(c->stream));
    HIPCHK(wait_stream(c));                                       // the first wait: how many entries, and which digits their keys differ in
    const size_t n = (size_t)c->sj.stat.h[SJ_ST_ENTRIES];
    if (n != cap) { snprintf(c->err, 512, "dg_sj_finish: the table holds %zu filled slots, %zu keys were counted", n, cap); return DG_ERR_INTERNAL; }
    const int bits1 = sj_key_bits(~c->sj.stat.h[SJ_ST_NMIN1], c->sj.stat.h[SJ_ST_MAX1]), bits2 = sj_key_bits(~c->sj.stat.h[SJ_ST_NMIN2], c->sj.stat.h[SJ_ST_MAX2]);
    int which = 0;
    HIPCHK(c->sj.sort.ensure((uint32_t)n));
    { const int rc = c->sj.sort.sort(c, (uint32_t)n, bits2, which); if (rc) return rc; }
    k_sj_gather<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(c->sj.tab, c->sj.sort.v[which].p, (uint32_t)n, c->sj.sort.k[which].p);
    { const int rc = c->sj.sort.sort(c, (uint32_t)n, bits1, which); if (rc) return rc; }
    SjPrint pr; pr.loc_key = c->ix.loc_key; pr.loc_chr = c->ix.loc_chr; pr.chr_off = c->ix.chr_off; pr.n2 = 2 * c->ix.n_chr; pr.name_off = nullptr; pr.names = nullptr;
    size_t text_cap = 0;
    {   // the chromosome names are read and the kernels that use them enqueued under the index's lock (as the SAM formatter does: dg_set_chr_names waits for the device before it frees them)
        std::unique_lock<std::mutex> lk;
        if (text) {
            lk = std::unique_lock<std::mutex>(sh->mu);
            pr.name_off = sh->d_chr_name_off; pr.names = sh->d_chr_names;
            text_cap = n * ((size_t)sh->chr_name_max + 3 * 21 + 4);      // a name, three numbers of at most 20 characters and a sign, three tabs and the line end
            HIPCHK(c->sj.text.ensure(text_cap));
        }
        k_sj_entries<<<n_tiles, SJ_THREADS, 0, c->stream>>>(c->sj.tab, c->sj.sort.v[which].p, (uint32_t)n, pr, c->sj.entries.p, c->sj.line_off.p, c->sj.tile.p, c->sj.stat.d);
        if (text) {
            k_tiles_top<uint64_t><<<1, 256, 0, c->stream>>>(c->sj.tile.p, n_tiles, (uint64_t *)(c->sj.stat.d + SJ_ST_BYTES));
            k_sj_write<<<n_tiles, SJ_THREADS, 0, c->stream>>>(c->sj.entries.p, (uint32_t)n, pr, c->sj.line_off.p, c->sj.tile.p, c->sj.stat.d, (unsigned long long)c->sj.text.cap, c->sj.text.p);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->sj.ev[1], c->stream));
    }
    HIPCHK(c->sj.stat.fetch(c->stream));
    HIPCHK(wait_stream(c));                                       // the second wait: lines and bytes
    const size_t bytes = text ? (size_t)c->sj.stat.h[SJ_ST_BYTES] : 0;
    if (bytes > c->sj.text.cap) { snprintf(c->err, 512, "dg_sj_finish: the text needs %zu bytes, the bound was %zu", bytes, c->sj.text.cap); return DG_ERR_INTERNAL; }
    const float ms = c->sj.ev.ms(0, 1);
    c->sj.fin_entries = n; c->sj.fin_bytes = bytes; c->sj.fin_valid = true;
    if (n_entries) *n_entries = n;
    if (n_lines) *n_lines = (size_t)c->sj.stat.h[SJ_ST_LINES];
    if (n_bytes) *n_bytes = bytes;
    if (device_ms) *device_ms = ms;
    return DG_OK;
}

extern "C" int dg_sj_download(dg_ctx *c, dg_sj_entry *entries, size_t cap_entries, char *text, size_t cap_text)
{
    if (!c) return DG_ERR_ARG;
    if (!c->sj.fin_valid) { snprintf(c->err, 512, "dg_sj_download: no finished table (dg_sj_finish first)"); return DG_ERR_ARG; }
    if ((entries && cap_entries < c->sj.fin_entries) || (text && cap_text < c->sj.fin_bytes)) {
        snprintf(c->err, 512, "dg_sj_download: output capacity too small: %zu entries and %zu bytes of text are needed", c->sj.fin_entries, c->sj.fin_bytes);
        return DG_ERR_CAPACITY;
    }
    HIPCHK(hipSetDevice(c->device));
    if (entries && c->sj.fin_entries) HIPCHK(hipMemcpyAsync(entries, c->sj.entries.p, c->sj.fin_entries * sizeof(dg_sj_entry), hipMemcpyDeviceToHost, c->stream));
    if (text && c->sj.fin_bytes) HIPCHK(hipMemcpyAsync(text, c->sj.text.p, c->sj.fin_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));
    return DG_OK;
}

extern "C" int dg_sj_device(dg_ctx *c, void **entries, void **text)
{
    if (!c) return DG_ERR_ARG;
    if (!c->sj.fin_valid) { snprintf(c->err, 512, "dg_sj_device: no finished table (dg_sj_finish first)"); return DG_ERR_ARG; }
    if (entries) *entries = c->sj.fin_entries ? c->sj.entries.p : nullptr;
    if (text) *text = c->sj.fin_bytes ? c->sj.text.p : nullptr;
    return DG_OK;
}

// ------------------------------------------------------------------------------------------
// coordinate-sorted BAM on the device (dg_bamsort.h): the records of every batch stay in HBM, one sort and one gather at the end of the job
// ------------------------------------------------------------------------------------------
static int bs_ready(dg_ctx *c)
{
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->bs.ready());
    HIPCHK(c->bam.ready());
    return DG_OK;
}
// One array of the store with room for `need` elements (`pad` more are allocated and never counted).  DBuf::ensure frees what it holds; here the first `used`
// elements are kept: allocate, copy device to device on the context's stream, wait, free.  hipMalloc fails: DG_ERR_CAPACITY, the array stays as it was.
template <typename T>
static int bs_grow(dg_ctx *c, T *&p, size_t &cap, size_t used, size_t need, size_t first, size_t pad, const char *fn, const char *what)
{
    if (need <= cap) return DG_OK;
    const size_t want = std::max(need, cap ? cap * 2 : first);
    T *q = nullptr;
    if (hipMalloc((void **)&q, (want + pad) * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        snprintf(c->err, 512, "%s: the store cannot grow: its %s need %zu bytes of device memory (%zu are held)", fn, what, (want + pad) * sizeof(T), cap ? (cap + pad) * sizeof(T) : (size_t)0);
        return DG_ERR_CAPACITY;
    }
    hipError_t e = hipSuccess;
    if (p && used) e = hipMemcpyAsync(q, p, used * sizeof(T), hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess && p) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void)hipFree(q); return fail(c, DG_ERR_HIP, "growing the sorted-BAM store", e); }
    if (p) (void)hipFree(p);
    p = q; cap = want;
    return DG_OK;
}
// room for n_rec more records of `bytes` bytes
static int bs_reserve(dg_ctx *c, size_t n_rec, size_t bytes, const char *fn)
{
    if (c->bs.n + n_rec >= 0xFFFFF000ull) { snprintf(c->err, 512, "%s: %zu records are more than the sorter takes", fn, c->bs.n + n_rec); return DG_ERR_ARG; }
    const size_t hook = c->bs.first_cap;
    const size_t first_bytes = hook ? std::max<size_t>(hook, BS_MIN_BYTES) : (size_t)1 << 24, first_recs = hook ? std::max<size_t>(hook / 64, 16) : (size_t)1 << 16;
    const bool grows = (c->bs.rec && c->bs.rec_used + bytes > c->bs.rec_cap) || (c->bs.key && c->bs.n + n_rec > c->bs.key_cap);      // an array is replaced by a larger one
    int rc = bs_grow(c, c->bs.rec, c->bs.rec_cap, c->bs.rec_used, c->bs.rec_used + bytes, first_bytes, 8, fn, "records");
    if (!rc) rc = bs_grow(c, c->bs.key, c->bs.key_cap, c->bs.n, c->bs.n + n_rec, first_recs, 0, fn, "keys");
    if (!rc) rc = bs_grow(c, c->bs.off, c->bs.off_cap, c->bs.n, c->bs.n + n_rec, first_recs, 0, fn, "offsets");
    if (!rc && grows) c->bs.growths++;
    return rc;
}
static void bs_commit(dg_ctx *c, uint32_t ordinal, size_t n_rec, size_t bytes)
{
    c->bs.segs.push_back(BsSeg{ordinal, (uint64_t)c->bs.n, (uint64_t)n_rec});
    c->bs.n += n_rec; c->bs.rec_used += bytes;
}
#define BS_ENSURE(buf, n, what) do { if ((buf).ensure(n) != hipSuccess) { (void)hipGetLastError(); \
    snprintf(c->err, 512, "%s: not enough device memory: %s need %zu bytes", fn, what, (size_t)(n) * sizeof(*(buf).p)); return DG_ERR_CAPACITY; } } while (0)
// the same for the scratch of a sort of n pairs (SortBufs::ensure names the array it could not have)
#define BS_ENSURE_SORT(sb, n) do { if ((sb).ensure(n) != hipSuccess) { (void)hipGetLastError(); \
    snprintf(c->err, 512, "%s: not enough device memory: %s need %zu bytes", fn, (sb).short_of, (sb).short_bytes); return DG_ERR_CAPACITY; } } while (0)

// The sorted array as the stages behind dg_bam_sort_finish read it (index, coverage, duplicate marking): the records' bytes, every record's place inside its
// tile (the sorter's other key buffer) and the tiles' sums.  bs_view is those stages' common beginning: a sorted array must be there.
struct BsView { unsigned char *rec; const uint64_t *dst_off; uint64_t *tile; size_t n, n_raw; int n_chr; };
static int bs_view(dg_ctx *c, const char *fn, BsView &v)
{
    if (!c->bs.fin_valid) { snprintf(c->err, 512, "%s: no sorted array (dg_bam_sort_finish first, and no store call behind it)", fn); return DG_ERR_ARG; }
    { const int rc = bs_ready(c); if (rc) return rc; }
    v.rec = c->bs.sorted.p; v.dst_off = c->bs.sort.k[c->bs.fin_which ^ 1].p; v.tile = c->bs.tile.p;
    v.n = c->bs.fin_records; v.n_raw = c->bs.fin_bytes; v.n_chr = c->ix.n_chr;
    return DG_OK;
}
// the bytes of the sorted array changed (a new sort, duplicate flags written): no block of it has been compressed, and no index or track covers it
static void bs_array_changed(dg_ctx *c) { c->bi.valid = false; c->bi.covered.clear(); c->cv.valid = false; c->pu.valid = false; c->qc.valid = false; c->rm.valid = false; }

extern "C" int dg_bam_sort_granules(int out[3])
{
    if (!out) return DG_ERR_ARG;
    out[0] = BS_THREADS; out[1] = RS_TILE; out[2] = BS_MIN_BYTES;
    return DG_OK;
}

// test hook (not in the public header): [0] records, [1] bytes, [2] segments, [3] the calls in which the store grew (an array replaced by a larger one)
extern "C" int dg_bam_sort_info(dg_ctx *c, size_t out[4])
{
    if (!c || !out) return DG_ERR_ARG;
    out[0] = c->bs.n; out[1] = c->bs.rec_used; out[2] = c->bs.segs.size(); out[3] = c->bs.growths;
    return DG_OK;
}

extern "C" int dg_bam_sort_reset(dg_ctx *c)
{
    if (!c) return DG_ERR_ARG;
    { const int rc = bs_ready(c); if (rc) return rc; }
    HIPCHK(wait_stream(c));
    c->bs.n = 0; c->bs.rec_used = 0; c->bs.segs.clear(); c->bs.fin_valid = false;
    return DG_OK;
}

extern "C" int dg_batch_accumulate_bam(dg_ctx *c, uint32_t ordinal, size_t *n_records, size_t *n_bytes)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_batch_accumulate_bam";
    if (n_records) *n_records = 0;
    if (n_bytes) *n_bytes = 0;
    if (!c->bam.rec_valid) { snprintf(c->err, 512, "%s: the records of the current batch are not there (dg_batch_format_bam on a finished batch first, and no dg_batch_format_sam behind it)", fn); return DG_ERR_ARG; }
    if (c->bam.rec_stored) { snprintf(c->err, 512, "%s: the records of this batch are in the store already (a batch is added once)", fn); return DG_ERR_ARG; }
    { const int rc = bs_ready(c); if (rc) return rc; }
    const size_t n_rec = c->bam.rec_records, bytes = c->bam.rec_bytes;
    if (!n_rec) { c->bam.rec_stored = true; return DG_OK; }
    { const int rc = bs_reserve(c, n_rec, bytes, fn); if (rc) return rc; }
    c->bs.fin_valid = false;
    const int n = c->n_reads;
    const uint32_t n_tiles = (uint32_t)((n + BS_THREADS - 1) / BS_THREADS);
    BS_ENSURE(c->bs.cnt_off, (size_t)n, "the per-read counts"); BS_ENSURE(c->bs.tile_cnt, (size_t)n_tiles + 1, "the per-workgroup counts");
    HIPCHK(hipEventRecord(c->bs.ev[0], c->stream));
    k_bs_count<<<n_tiles, BS_THREADS, 0, c->stream>>>(c->bam.rec.p, c->sam.read_off.p, c->sam.tile.p, n, (unsigned long long)bytes, c->bs.cnt_off.p, c->bs.tile_cnt.p);
    k_tiles_top<uint32_t><<<1, 256, 0, c->stream>>>(c->bs.tile_cnt.p, n_tiles, (uint32_t *)(c->bs.stat.d + 1));
    k_bs_emit<<<n_tiles, BS_THREADS, 0, c->stream>>>(c->bam.rec.p, c->sam.read_off.p, c->sam.tile.p, n, (unsigned long long)bytes, c->bs.cnt_off.p, c->bs.tile_cnt.p, c->ix.n_chr,
                                                     (unsigned long long)c->bs.n, (unsigned long long)(c->bs.n + n_rec), (unsigned long long)c->bs.rec_used, c->bs.key, c->bs.off);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->bs.rec + c->bs.rec_used, c->bam.rec.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipEventRecord(c->bs.ev[1], c->stream));
    HIPCHK(hipMemcpyAsync(c->bs.stat.h + 1, c->bs.stat.d + 1, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));                                       // the one wait: the walk must find the records the formatter counted
    c->bs.acc_ms = c->bs.ev.ms(0, 1);
    const size_t found = (size_t)(uint32_t)c->bs.stat.h[1];
    if (found != n_rec) { snprintf(c->err, 512, "%s: the walk over the batch's records found %zu, the formatter wrote %zu; nothing was added", fn, found, n_rec); return DG_ERR_INTERNAL; }
    bs_commit(c, ordinal, n_rec, bytes);
    c->bam.rec_stored = true;
    if (n_records) *n_records = n_rec;
    if (n_bytes) *n_bytes = bytes;
    return DG_OK;
}

extern "C" int dg_bam_sort_add(dg_ctx *c, const void *records, size_t n, uint32_t ordinal, size_t *n_records)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_bam_sort_add";
    if (n_records) *n_records = 0;
    if (n && !records) { snprintf(c->err, 512, "%s: the input is NULL", fn); return DG_ERR_ARG; }
    { const int rc = bs_ready(c); if (rc) return rc; }
    if (!n) return DG_OK;
    const unsigned char *p = (const unsigned char *)records;
    const int n_chr = c->ix.n_chr;
    const uint64_t base = c->bs.rec_used;
    std::vector<uint64_t> keys; std::vector<int64_t> offs;
    size_t bad = 0; int why = BS_REC_OK;
    const size_t n_rec = bs_walk_checked(p, n, n_chr, &bad, &why, [&](size_t, size_t at) { keys.push_back(bs_key(p + at, n_chr)); offs.push_back((int64_t)(base + at)); });
    if (why) { snprintf(c->err, 512, "%s: record %zu: %s; nothing was added", fn, bad, bs_rec_why(why)); return DG_ERR_ARG; }
    { const int rc = bs_reserve(c, n_rec, n, fn); if (rc) return rc; }
    c->bs.fin_valid = false;
    HIPCHK(hipMemcpyAsync(c->bs.rec + c->bs.rec_used, p, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->bs.key + c->bs.n, keys.data(), n_rec * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->bs.off + c->bs.n, offs.data(), n_rec * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(wait_stream(c));
    bs_commit(c, ordinal, n_rec, n);
    if (n_records) *n_records = n_rec;
    return DG_OK;
}

extern "C" int dg_bam_sort_merge(dg_ctx *dst, dg_ctx *src)
{
    dg_ctx *c = dst;
    if (!dst || !src) return DG_ERR_ARG;
    const char *fn = "dg_bam_sort_merge";
    if (dst == src || dst->device != src->device) { snprintf(c->err, 512, "%s: the two contexts must differ and be on one device", fn); return DG_ERR_ARG; }
    { const int rc = bs_ready(dst); if (rc) return rc; }
    if (!src->bs.n) { src->bs.fin_valid = false; return DG_OK; }
    HIPCHK(src->bs.ready());
    const size_t n_rec = src->bs.n, bytes = src->bs.rec_used;
    { const int rc = bs_reserve(dst, n_rec, bytes, fn); if (rc) return rc; }
    dst->bs.fin_valid = false; src->bs.fin_valid = false;
    // behind everything the source's stream holds; the call waits for the destination's stream, so the source's storage is free again when it returns
    HIPCHK(hipEventRecord(src->bs.ev[5], src->stream));
    HIPCHK(hipStreamWaitEvent(dst->stream, src->bs.ev[5], 0));
    HIPCHK(hipMemcpyAsync(dst->bs.rec + dst->bs.rec_used, src->bs.rec, bytes, hipMemcpyDeviceToDevice, dst->stream));
    HIPCHK(hipMemcpyAsync(dst->bs.key + dst->bs.n, src->bs.key, n_rec * 8, hipMemcpyDeviceToDevice, dst->stream));
    k_bs_shift<<<(unsigned)((n_rec + 255) / 256), 256, 0, dst->stream>>>(src->bs.off, dst->bs.off + dst->bs.n, (unsigned long long)n_rec, (long long)dst->bs.rec_used);
    HIPCHK(hipGetLastError());
    HIPCHK(wait_stream(dst));
    for (const BsSeg &s : src->bs.segs) dst->bs.segs.push_back(BsSeg{s.ordinal, s.start + (uint64_t)dst->bs.n, s.count});      // behind dst's own: among equal ordinals dst's come first
    dst->bs.n += n_rec; dst->bs.rec_used += bytes;
    src->bs.n = 0; src->bs.rec_used = 0; src->bs.segs.clear();
    return DG_OK;
}

extern "C" int dg_bam_sort_finish(dg_ctx *c, size_t *n_records, size_t *n_raw, float *device_ms)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_bam_sort_finish";
    if (n_records) *n_records = 0;
    if (n_raw) *n_raw = 0;
    if (device_ms) *device_ms = 0.f;
    c->bs.fin_valid = false; c->bs.fin_bytes = 0; c->bs.fin_records = 0; c->bs.passes = 0;
    bs_array_changed(c);
    for (float &m : c->bs.ms) m = 0.f;
    { const int rc = bs_ready(c); if (rc) return rc; }
    if (!c->bs.n) { c->bs.fin_valid = true; return DG_OK; }
    const size_t n = c->bs.n, bytes = c->bs.rec_used;
    const uint32_t n_tiles = (uint32_t)((n + BS_THREADS - 1) / BS_THREADS);
    for (int k = 0; k < 2; k++) { BS_ENSURE(c->bs.sort.k[k], n, "the sorter's keys"); BS_ENSURE(c->bs.sort.v[k], n, "the sorter's values"); }
    BS_ENSURE(c->bs.tile, (size_t)n_tiles, "the per-workgroup sums"); BS_ENSURE(c->bs.sorted, bytes + 8, "the sorted records");
    // step one: the segments in ordinal order (neighbours in the store that stay neighbours go in one copy)
    std::vector<uint32_t> order(c->bs.segs.size());
    bs_order_segments(c->bs.segs.data(), c->bs.segs.size(), order.data());
    HIPCHK(hipEventRecord(c->bs.ev[0], c->stream));
    size_t at = 0;
    for (size_t i = 0; i < order.size();) {
        const uint64_t start = c->bs.segs[order[i]].start;
        uint64_t count = c->bs.segs[order[i]].count;
        for (i++; i < order.size() && c->bs.segs[order[i]].start == start + count; i++) count += c->bs.segs[order[i]].count;
        if (!count) continue;
        HIPCHK(hipMemcpyAsync(c->bs.sort.k[0].p + at, c->bs.key + start, count * 8, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->bs.sort.v[0].p + at, c->bs.off + start, count * 8, hipMemcpyDeviceToDevice, c->stream));
        at += count;
    }
    if (at != n) { snprintf(c->err, 512, "%s: the segments hold %zu records, the store %zu", fn, at, n); return DG_ERR_INTERNAL; }
    HIPCHK(hipEventRecord(c->bs.ev[1], c->stream));
    // step two: one stable sort; the values are the records' offsets in the store
    int which = 0;
    const int bits = bs_key_bits(c->ix.n_chr);
    BS_ENSURE_SORT(c->bs.sort, (uint32_t)n);
    { const int rc = c->bs.sort.sort(c, (uint32_t)n, bits, which); if (rc) return rc; }
    c->bs.passes = (bits + 3) / 4;
    HIPCHK(hipEventRecord(c->bs.ev[2], c->stream));
    // step three: lengths in sorted order, their scan (the places go where the sorter's other key buffer was), the gather
    uint64_t *dst_off = c->bs.sort.k[which ^ 1].p;
    k_bs_len<<<n_tiles, BS_THREADS, 0, c->stream>>>(c->bs.rec, c->bs.sort.v[which].p, (uint32_t)n, dst_off, c->bs.tile.p);
    k_tiles_top<uint64_t><<<1, 256, 0, c->stream>>>(c->bs.tile.p, n_tiles, (uint64_t *)c->bs.stat.d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->bs.ev[3], c->stream));
    k_bs_gather<<<(unsigned)((n + BS_GATHER_WAVES - 1) / BS_GATHER_WAVES), 64 * BS_GATHER_WAVES, 0, c->stream>>>(c->bs.rec, c->bs.sort.v[which].p, dst_off, c->bs.tile.p, (uint32_t)n,
                                                                                                             (unsigned long long)bytes, c->bs.sorted.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->bs.ev[4], c->stream));
    HIPCHK(hipMemcpyAsync(c->bs.stat.h, c->bs.stat.d, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));
    if ((size_t)c->bs.stat.h[0] != bytes) { snprintf(c->err, 512, "%s: the sorted records' lengths add up to %zu bytes, the store holds %zu", fn, (size_t)c->bs.stat.h[0], bytes); return DG_ERR_INTERNAL; }
    float total = 0.f;
    for (int k = 0; k < 4; k++) { c->bs.ms[k] = c->bs.ev.ms(k, k + 1); total += c->bs.ms[k]; }
    c->bs.fin_valid = true; c->bs.fin_bytes = bytes; c->bs.fin_records = n; c->bs.fin_which = which;
    if (n_records) *n_records = n;
    if (n_raw) *n_raw = bytes;
    if (device_ms) *device_ms = total;
    return DG_OK;
}

extern "C" int dg_bam_sort_device_ms(dg_ctx *c, float ms[5], int *n_passes)
{
    if (!c || !ms) return DG_ERR_ARG;
    for (int k = 0; k < 4; k++) ms[k] = c->bs.ms[k];
    ms[4] = c->bs.acc_ms;
    if (n_passes) *n_passes = c->bs.passes;
    return DG_OK;
}

extern "C" int dg_bam_sort_device(dg_ctx *c, void **ptr, size_t *n_raw)
{
    if (!c || !ptr || !n_raw) return DG_ERR_ARG;
    if (!c->bs.fin_valid) { snprintf(c->err, 512, "dg_bam_sort_device: no sorted array (dg_bam_sort_finish first)"); return DG_ERR_ARG; }
    *ptr = c->bs.fin_bytes ? c->bs.sorted.p : nullptr; *n_raw = c->bs.fin_bytes;
    return DG_OK;
}

extern "C" int dg_bam_sort_compress(dg_ctx *c, size_t raw_off, size_t raw_len, uint32_t flags, size_t *n_bytes, float *device_ms)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_bam_sort_compress";
    if (n_bytes) *n_bytes = 0;
    if (device_ms) *device_ms = 0.f;
    c->bam.valid = false; c->bam.bytes = 0; c->bam.ptr = nullptr;
    if (!c->bs.fin_valid) { snprintf(c->err, 512, "%s: no sorted array (dg_bam_sort_finish first, and no store call behind it)", fn); return DG_ERR_ARG; }
    if (flags != 0u && flags != DG_BGZF_DYNAMIC && flags != DG_BAM_RAW) { snprintf(c->err, 512, "%s: flags 0x%x are none of 0, DG_BGZF_DYNAMIC, DG_BAM_RAW", fn, flags); return DG_ERR_ARG; }
    const size_t total = c->bs.fin_bytes;
    if (raw_off % BGZF_BLOCK || raw_off > total || raw_len > total - raw_off || (raw_len % BGZF_BLOCK && raw_off + raw_len != total)) {
        snprintf(c->err, 512, "%s: the range %zu + %zu of %zu bytes must begin at a multiple of %u, and end at one or at the array's end", fn, raw_off, raw_len, total, BGZF_BLOCK);
        return DG_ERR_ARG;
    }
    if (!raw_len) { c->bam.valid = true; return DG_OK; }
    { const int rc = bs_ready(c); if (rc) return rc; }
    unsigned char *in = c->bs.sorted.p + raw_off;
    size_t out_bytes = raw_len; float ms = 0.f;
    c->bam.ptr = in;
    if (flags != DG_BAM_RAW) {
        const int rc = bgzf_device(c, in, raw_len, flags == DG_BGZF_DYNAMIC, &out_bytes, &ms);
        if (rc) return rc;
        c->bam.ptr = c->bam.bgzf_out.p;
        // the blocks' compressed sizes, kept for dg_bam_index_finish: device to device, at the piece's block offset
        const size_t all_blocks = (total + BGZF_BLOCK - 1) / BGZF_BLOCK, b0 = raw_off / BGZF_BLOCK, nb = (raw_len + BGZF_BLOCK - 1) / BGZF_BLOCK;
        // (no memory for that array: the compression stands, the blocks stay uncovered, and dg_bam_index_finish without block_sizes says which block it misses)
        if (c->bi.sizes.cap < all_blocks) { c->bi.covered.clear(); if (c->bi.sizes.ensure(all_blocks) != hipSuccess) (void)hipGetLastError(); }
        if (c->bi.sizes.cap >= all_blocks) {
            if (c->bi.covered.size() != all_blocks) c->bi.covered.assign(all_blocks, 0);
            HIPCHK(hipMemcpyAsync(c->bi.sizes.p + b0, c->bam.bgzf_size.p, nb * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
            std::fill(c->bi.covered.begin() + (long)b0, c->bi.covered.begin() + (long)(b0 + nb), (unsigned char)1);
        }
    }
    c->bam.bytes = out_bytes; c->bam.valid = true;
    c->bam.ms[0] = 0.f; c->bam.ms[1] = ms;
    if (n_bytes) *n_bytes = out_bytes;
    if (device_ms) *device_ms = ms;
    return DG_OK;
}

// ------------------------------------------------------------------------------------------
// the BAM index of the sorted array (dg_bamidx.h): built in HBM from the sorted records, their places and the blocks' compressed sizes
// ------------------------------------------------------------------------------------------
extern "C" int dg_bam_index_granules(int out[2])
{
    if (!out) return DG_ERR_ARG;
    out[0] = BI_THREADS; out[1] = RS_TILE;
    return DG_OK;
}

extern "C" int dg_bam_index_finish(dg_ctx *c, uint64_t first_block_offset, const uint32_t *block_sizes, size_t n_blocks_given, size_t *n_bytes, uint64_t stats[6], float *device_ms)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_bam_index_finish";
    if (n_bytes) *n_bytes = 0;
    if (device_ms) *device_ms = 0.f;
    if (stats) for (int k = 0; k < 6; k++) stats[k] = 0;
    c->bi.valid = false; c->bi.bytes = 0;
    BsView sv;
    { const int rc = bs_view(c, fn, sv); if (rc) return rc; }
    HIPCHK(c->bi.ready());
    const size_t n = sv.n, n_raw = sv.n_raw, n_blocks = (n_raw + BGZF_BLOCK - 1) / BGZF_BLOCK;
    const int n_chr = sv.n_chr;
    if (n_chr < 1 || n_blocks > 0xFFFFFFF0ull) { snprintf(c->err, 512, "%s: %d chromosomes, %zu blocks", fn, n_chr, n_blocks); return DG_ERR_ARG; }
    if (first_block_offset >> 48) { snprintf(c->err, 512, "%s: the first block's file offset %llu does not fit a virtual offset's 48 bits", fn, (unsigned long long)first_block_offset); return DG_ERR_RANGE; }
    // the blocks' sizes: the caller's, or what the last dg_bam_sort_compress of every block left
    const uint32_t *sizes = nullptr;
    if (block_sizes) {
        if (n_blocks_given != n_blocks) { snprintf(c->err, 512, "%s: n_blocks is %zu, the sorted array of %zu bytes has %zu blocks of %u bytes", fn, n_blocks_given, n_raw, n_blocks, BGZF_BLOCK); return DG_ERR_ARG; }
        for (size_t k = 0; k < n_blocks; k++) if (!block_sizes[k]) { snprintf(c->err, 512, "%s: block %zu has the compressed size 0", fn, k); return DG_ERR_ARG; }
        BS_ENSURE(c->bi.sizes_in, n_blocks + 1, "the blocks' compressed sizes");
        if (n_blocks) HIPCHK(hipMemcpyAsync(c->bi.sizes_in.p, block_sizes, n_blocks * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        sizes = c->bi.sizes_in.p;
    } else {
        for (size_t k = 0; k < n_blocks; k++) if (k >= c->bi.covered.size() || !c->bi.covered[k]) {
            snprintf(c->err, 512, "%s: block %zu of the sorted array has not been compressed since dg_bam_sort_finish (dg_bam_sort_compress without DG_BAM_RAW), and no block_sizes are given", fn, k);
            return DG_ERR_ARG;
        }
        sizes = c->bi.sizes.p;
    }
    const uint32_t tiles = (uint32_t)((n + BI_THREADS - 1) / BI_THREADS);
    BS_ENSURE(c->bi.coff, n_blocks + 1, "the blocks' file offsets");
    BS_ENSURE(c->bi.key, n + 1, "the records' bins"); BS_ENSURE(c->bi.voff, n + 1, "the records' virtual offsets"); BS_ENSURE(c->bi.span, n + 1, "the records' windows");
    BS_ENSURE(c->bi.tile_cnt, (size_t)tiles + 1, "the per-workgroup chunk counts");
    BS_ENSURE(c->bi.ref, (size_t)BI_REF_PLANES * n_chr, "the per-reference values");
    BS_ENSURE(c->bi.ref_q, (size_t)n_chr + 1, "the per-reference chunk counts"); BS_ENSURE(c->bi.ref_b, (size_t)n_chr + 1, "the per-reference bin counts");
    BS_ENSURE(c->bi.ref_at, (size_t)n_chr + 1, "the per-reference byte offsets"); BS_ENSURE(c->bi.lin_at, (size_t)n_chr + 1, "the per-reference window offsets");
    c->bi.h_ref.resize((size_t)BI_REF_PLANES * n_chr); c->bi.h_lin_at.resize((size_t)n_chr + 1);
    HIPCHK(hipMemsetAsync(c->bi.stat.d, 0, BI_ST_WORDS * 8, c->stream));
    HIPCHK(hipMemsetAsync(c->bi.stat.d + BI_ST_BAD, 0xff, 8, c->stream));
    HIPCHK(hipMemsetAsync(c->bi.ref.p, 0, (size_t)BI_REF_PLANES * n_chr * 8, c->stream));
    HIPCHK(hipMemsetAsync(c->bi.ref.p + 3 * (size_t)n_chr, 0xff, (size_t)n_chr * 8, c->stream));
    HIPCHK(hipEventRecord(c->bi.ev[0], c->stream));
    k_bi_coff<<<1, BI_THREADS, 0, c->stream>>>(sizes, (uint32_t)n_blocks, (unsigned long long)first_block_offset, c->bi.coff.p, c->bi.stat.d);
    if (n) {
        k_bi_rec<<<tiles, BI_THREADS, 0, c->stream>>>(sv.rec, sv.dst_off, sv.tile, (uint32_t)n, (unsigned long long)n_raw, c->bi.coff.p, (uint32_t)n_blocks, n_chr,
                                                      c->bi.key.p, c->bi.voff.p, c->bi.span.p, c->bi.ref.p, c->bi.stat.d);
        k_bi_heads<<<tiles, BI_THREADS, 0, c->stream>>>(c->bi.key.p, (uint32_t)n, c->bi.tile_cnt.p);
        k_tiles_top<uint32_t><<<1, 256, 0, c->stream>>>(c->bi.tile_cnt.p, tiles, (uint32_t *)(c->bi.stat.d + BI_ST_CHUNKS));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->bi.ev[1], c->stream));
    HIPCHK(c->bi.stat.fetch(c->stream));
    HIPCHK(hipMemcpyAsync(c->bi.h_ref.data(), c->bi.ref.p, (size_t)BI_REF_PLANES * n_chr * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));                                       // the first wait: the per-reference sizes (and the chunk count, and what was out of range)
    if (c->bi.stat.h[BI_ST_COFF_END] >> 48) { snprintf(c->err, 512, "%s: the file offset %llu behind the last block does not fit a virtual offset's 48 bits", fn, c->bi.stat.h[BI_ST_COFF_END]); return DG_ERR_RANGE; }
    if (c->bi.stat.h[BI_ST_BAD] != BI_NONE) {
        snprintf(c->err, 512, "%s: record %llu of the sorted array ends behind position 2^29: a BAI cannot hold it, such a reference needs a CSI index; no index was built", fn, c->bi.stat.h[BI_ST_BAD]);
        return DG_ERR_RANGE;
    }
    const size_t n_chunks = (size_t)(uint32_t)c->bi.stat.h[BI_ST_CHUNKS];
    size_t n_placed = 0, n_lin = 0;
    for (int t = 0; t < n_chr; t++) {
        c->bi.h_lin_at[(size_t)t] = n_lin;
        n_lin += (size_t)c->bi.h_ref[(size_t)t];
        n_placed += (size_t)(c->bi.h_ref[(size_t)n_chr + t] + c->bi.h_ref[2 * (size_t)n_chr + t]);
    }
    c->bi.h_lin_at[(size_t)n_chr] = n_lin;
    if (n_placed > n || n_chunks > n_placed) { snprintf(c->err, 512, "%s: %zu placed records and %zu chunks of %zu records", fn, n_placed, n_chunks, n); return DG_ERR_INTERNAL; }
    const size_t cap = (size_t)bi_bytes_bound((uint64_t)n_chr, n_chunks, n_lin);
    const uint32_t ctiles = (uint32_t)((n_chunks + BI_THREADS - 1) / BI_THREADS);
    BS_ENSURE(c->bi.lin, n_lin + 1, "the linear index"); BS_ENSURE(c->bi.out, cap, "the index");
    for (int k = 0; k < 2; k++) { BS_ENSURE(c->bi.sort.k[k], n_chunks + 1, "the chunks' keys"); BS_ENSURE(c->bi.sort.v[k], n_chunks + 1, "the chunks' numbers"); }
    BS_ENSURE(c->bi.chead, n_chunks + 1, "the chunks' first records"); BS_ENSURE(c->bi.mhead, n_chunks + 1, "the merged chunks"); BS_ENSURE(c->bi.mbin, n_chunks + 1, "the merged chunks' bins");
    BS_ENSURE(c->bi.binq, n_chunks + 1, "the bins' first chunks"); BS_ENSURE(c->bi.flag, n_chunks + 1, "the chunks' flags"); BS_ENSURE(c->bi.excl, n_chunks + 1, "the chunks' places");
    BS_ENSURE(c->bi.ctile, (size_t)ctiles + 1, "the per-workgroup sums");
    BS_ENSURE_SORT(c->bi.sort, (uint32_t)n_chunks);
    HIPCHK(hipMemcpyAsync(c->bi.lin_at.p, c->bi.h_lin_at.data(), ((size_t)n_chr + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->bi.ev[2], c->stream));
    HIPCHK(hipMemsetAsync(c->bi.out.p, 0, cap, c->stream));
    if (n_lin) {
        HIPCHK(hipMemsetAsync(c->bi.lin.p, 0xff, n_lin * 8, c->stream));
        k_bi_lin<<<tiles, BI_THREADS, 0, c->stream>>>(c->bi.key.p, c->bi.span.p, c->bi.voff.p, (uint32_t)n, n_chr, c->bi.lin_at.p, c->bi.lin.p);
    }
    int which = 0;
    if (n_chunks) {
        k_bi_chunks<<<tiles, BI_THREADS, 0, c->stream>>>(c->bi.key.p, (uint32_t)n, c->bi.tile_cnt.p, (uint32_t)n_chunks, (uint32_t)n_placed, c->bi.sort.k[0].p, c->bi.sort.v[0].p, c->bi.chead.p);
        { const int rc = c->bi.sort.sort(c, (uint32_t)n_chunks, bi_key_bits(n_chr), which); if (rc) return rc; }
        k_bi_merge_scan<<<ctiles, BI_THREADS, 0, c->stream>>>(c->bi.sort.k[which].p, c->bi.sort.v[which].p, c->bi.chead.p, c->bi.voff.p, (uint32_t)n_chunks, c->bi.flag.p, c->bi.excl.p, c->bi.ctile.p);
        k_tiles_top<uint64_t><<<1, 256, 0, c->stream>>>(c->bi.ctile.p, ctiles, (uint64_t *)(c->bi.stat.d + BI_ST_MERGED));
        k_bi_merge_emit<<<ctiles, BI_THREADS, 0, c->stream>>>(c->bi.sort.k[which].p, c->bi.flag.p, c->bi.excl.p, c->bi.ctile.p, (uint32_t)n_chunks, n_chr, c->bi.stat.d, c->bi.mhead.p, c->bi.mbin.p,
                                                               c->bi.binq.p, c->bi.ref_q.p, c->bi.ref_b.p);
    } else {
        HIPCHK(hipMemsetAsync(c->bi.ref_q.p, 0, ((size_t)n_chr + 1) * 4, c->stream));
        HIPCHK(hipMemsetAsync(c->bi.ref_b.p, 0, ((size_t)n_chr + 1) * 4, c->stream));
    }
    k_bi_refs<<<1, BI_THREADS, 0, c->stream>>>(n_chr, c->bi.ref.p, c->bi.ref_q.p, c->bi.ref_b.p, (unsigned long long)(n - n_placed), c->bi.ref_at.p, c->bi.out.p, (unsigned long long)cap, c->bi.stat.d);
    if (n_chunks)
        k_bi_write_chunks<<<ctiles, BI_THREADS, 0, c->stream>>>(c->bi.sort.k[which].p, c->bi.sort.v[which].p, c->bi.chead.p, c->bi.voff.p, (uint32_t)n_chunks, c->bi.stat.d, c->bi.mhead.p, c->bi.mbin.p,
                                                                 c->bi.binq.p, c->bi.ref_q.p, c->bi.ref_b.p, c->bi.ref_at.p, n_chr, c->bi.out.p, (unsigned long long)cap);
    k_bi_write_refs<<<(unsigned)n_chr, BI_THREADS, 0, c->stream>>>(n_chr, c->bi.ref.p, c->bi.ref_q.p, c->bi.ref_b.p, c->bi.ref_at.p, c->bi.voff.p, (uint32_t)n, c->bi.lin_at.p, c->bi.lin.p,
                                                                   c->bi.out.p, (unsigned long long)cap);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->bi.ev[3], c->stream));
    HIPCHK(c->bi.stat.fetch(c->stream));
    HIPCHK(wait_stream(c));                                       // the second wait: the index's size
    const size_t total = (size_t)c->bi.stat.h[BI_ST_BYTES], n_merged = (size_t)(uint32_t)c->bi.stat.h[BI_ST_MERGED], n_bins = (size_t)(c->bi.stat.h[BI_ST_MERGED] >> 32);
    if (total > cap || total < 16 + 8 * (size_t)n_chr || n_merged > n_chunks || n_bins > n_merged) {
        snprintf(c->err, 512, "%s: an index of %zu bytes (%zu chunks, %zu bins) where at most %zu bytes and %zu chunks can be", fn, total, n_merged, n_bins, cap, n_chunks);
        return DG_ERR_INTERNAL;
    }
    const float a = c->bi.ev.ms(0, 1), b = c->bi.ev.ms(2, 3);
    c->bi.valid = true; c->bi.bytes = total;
    if (n_bytes) *n_bytes = total;
    if (device_ms) *device_ms = a + b;
    if (stats) { stats[0] = n_placed; stats[1] = n - n_placed; stats[2] = n_bins; stats[3] = n_chunks; stats[4] = n_merged; stats[5] = n_lin; }
    return DG_OK;
}

extern "C" int dg_bam_index_download(dg_ctx *c, void *out, size_t cap)
{
    if (!c || (!out && cap)) return DG_ERR_ARG;
    if (!c->bi.valid || !c->bs.fin_valid) { snprintf(c->err, 512, "dg_bam_index_download: no index (dg_bam_index_finish first, and no store call behind it)"); return DG_ERR_ARG; }
    if (cap < c->bi.bytes) { snprintf(c->err, 512, "dg_bam_index_download: the index has %zu bytes, the buffer %zu", c->bi.bytes, cap); return DG_ERR_CAPACITY; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(out, c->bi.out.p, c->bi.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));
    return DG_OK;
}

extern "C" int dg_bam_index_device(dg_ctx *c, void **ptr, size_t *n_bytes)
{
    if (!c || !ptr || !n_bytes) return DG_ERR_ARG;
    if (!c->bi.valid || !c->bs.fin_valid) { snprintf(c->err, 512, "dg_bam_index_device: no index (dg_bam_index_finish first, and no store call behind it)"); return DG_ERR_ARG; }
    *ptr = c->bi.out.p; *n_bytes = c->bi.bytes;
    return DG_OK;
}

// ------------------------------------------------------------------------------------------
// gene-level read counts (dg_genecount.h): the annotation's segment table lives with the index, a table of counts with every context
// ------------------------------------------------------------------------------------------
extern "C" int dg_gene_granules(int out[2])
{
    if (!out) return DG_ERR_ARG;
    out[0] = GC_THREADS; out[1] = GC_WAVE;
    return DG_OK;
}

extern "C" int dg_gene_set_annotation(dg_ctx *c, const dg_gene_annot *a, size_t *n_segments)
{
    if (!c) return DG_ERR_ARG;
    if (n_segments) *n_segments = 0;
    IndexShared *sh = c->shared_ix;
    if (!sh || !a) { snprintf(c->err, 512, "dg_gene_set_annotation: no annotation (or a context without an index)"); return DG_ERR_ARG; }
    std::vector<uint32_t> chr_first, seg_start, seg_lab;
    char why[400];
    if (!gc_flatten(c->ix.n_chr, a->n_genes, a->n_exons, a->exons, chr_first, seg_start, seg_lab, why, sizeof why)) { snprintf(c->err, 512, "dg_gene_set_annotation: %s", why); return DG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(sh->mu);
    uint32_t *d[3] = {nullptr, nullptr, nullptr};
    const std::vector<uint32_t> *src[3] = {&chr_first, &seg_start, &seg_lab};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 3 && e == hipSuccess; k++) {
        e = hipMalloc((void **)&d[k], (src[k]->size() + 1) * 4);
        if (e == hipSuccess && !src[k]->empty()) e = hipMemcpy(d[k], src[k]->data(), src[k]->size() * 4, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) { for (uint32_t *p : d) if (p) (void)hipFree(p); return fail(c, DG_ERR_HIP, "the gene annotation's segment table", e); }
    // A count of any context of this index reads the three pointers and enqueues its kernels under sh->mu, so under the lock every kernel that may read the
    // old table is already in a stream: the device is waited for, then it is freed (as dg_set_chr_names does).
    if (sh->gc_gen) { (void)hipDeviceSynchronize(); (void)hipFree(sh->d_gc_chr_first); (void)hipFree(sh->d_gc_seg_start); (void)hipFree(sh->d_gc_seg_lab); }
    sh->d_gc_chr_first = d[0]; sh->d_gc_seg_start = d[1]; sh->d_gc_seg_lab = d[2];
    sh->gc_n_genes = a->n_genes; sh->gc_n_seg = seg_start.size(); sh->gc_gen++;
    if (n_segments) *n_segments = seg_start.size();
    return DG_OK;
}

// the context's table for the current annotation: made on first use; an empty one of another generation is replaced, a filled one is the caller's to reset
static int gc_ready(dg_ctx *c, const char *fn, bool fresh = false)
{
    IndexShared *sh = c->shared_ix;
    uint64_t gen = 0; size_t rows = 0;
    if (sh) { std::lock_guard<std::mutex> lk(sh->mu); gen = sh->gc_gen; rows = 4 + (size_t)sh->gc_n_genes; }
    if (!gen) { snprintf(c->err, 512, "%s: no gene annotation (dg_gene_set_annotation first)", fn); return DG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->gc.ready());
    if (c->gc.counts && c->gc.gen == gen && !fresh) return DG_OK;
    if (c->gc.counts && c->gc.gen != gen && c->gc.nonempty && !fresh) {
        snprintf(c->err, 512, "%s: the table holds counts of annotation generation %llu, the annotation is generation %llu now (dg_gene_reset first)", fn, (unsigned long long)c->gc.gen, (unsigned long long)gen);
        return DG_ERR_ARG;
    }
    if (!c->gc.counts || c->gc.rows != rows) {
        unsigned long long *t = nullptr;
        HIPCHK(hipMalloc((void **)&t, rows * 3 * 8));
        if (c->gc.counts) { (void)hipStreamSynchronize(c->stream); (void)hipFree(c->gc.counts); }
        c->gc.counts = t; c->gc.rows = rows;
    }
    HIPCHK(hipMemsetAsync(c->gc.counts, 0, c->gc.rows * 3 * 8, c->stream));
    c->gc.gen = gen; c->gc.nonempty = false;
    return DG_OK;
}

// k_gc_count and k_gc_top over the records b holds in HBM, behind whatever the stream holds
static int gc_count_device(dg_ctx *c, GcBatch b, const char *fn)
{
    IndexShared *sh = c->shared_ix;
    const unsigned long long n_units = gc_units(b.n_reads, b.n_pair_mode);
    const unsigned long long n_wg = (n_units + GC_THREADS - 1) / GC_THREADS;
    if (!n_units) return DG_OK;
    if (n_wg > 0x7FFFFFFFull) { snprintf(c->err, 512, "%s: %llu units are more than one call takes", fn, n_units); return DG_ERR_ARG; }
    HIPCHK(c->gc.wg.ensure((size_t)n_wg * 12));
    std::lock_guard<std::mutex> lk(sh->mu);          // (dg_gene_set_annotation replaces the table under the same lock and waits for the device before it frees the old one)
    if (sh->gc_gen != c->gc.gen) { snprintf(c->err, 512, "%s: the annotation was replaced while the call was being prepared", fn); return DG_ERR_ARG; }
    const GcTable t{sh->d_gc_chr_first, sh->d_gc_seg_start, sh->d_gc_seg_lab, c->ix.n_chr};
    HIPCHK(hipEventRecord(c->gc.ev[0], c->stream));
    k_gc_count<<<(unsigned)n_wg, GC_THREADS, 0, c->stream>>>(b, t, n_units, c->gc.counts, (unsigned long long)c->gc.rows, c->gc.wg.p);
    k_gc_top<<<1, 256, 0, c->stream>>>(c->gc.wg.p, n_wg, c->gc.counts);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->gc.ev[1], c->stream));
    c->gc.timed = true; c->gc.nonempty = true;
    return DG_OK;
}

static int gc_pair_mode_ok(dg_ctx *c, const char *fn, int n_pair_mode, int n)
{
    if (n_pair_mode < 0 || (n_pair_mode & 1) || n_pair_mode > n) { snprintf(c->err, 512, "%s: n_pair_mode %d must be even and at most the batch's %d reads", fn, n_pair_mode, n); return DG_ERR_ARG; }
    return DG_OK;
}

extern "C" int dg_batch_accumulate_genes(dg_ctx *c, int n_pair_mode, uint32_t min_mapq, size_t *n_units)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_batch_accumulate_genes";
    if (n_units) *n_units = 0;
    { IndexShared *sh = c->shared_ix; uint64_t gen = 0; if (sh) { std::lock_guard<std::mutex> lk(sh->mu); gen = sh->gc_gen; }
      if (!gen) { snprintf(c->err, 512, "%s: no gene annotation (dg_gene_set_annotation first)", fn); return DG_ERR_ARG; } }
    if (!c->batch_done) { snprintf(c->err, 512, "%s: the context has no finished batch (upload and run one first)", fn); return DG_ERR_ARG; }
    { const int rc = gc_pair_mode_ok(c, fn, n_pair_mode, c->n_reads); if (rc) return rc; }
    if (c->n_reads && !c->full_valid) { snprintf(c->err, 512, "%s: the last batch has no full records (it was mapped through dg_map_batch_compact)", fn); return DG_ERR_ARG; }
    if (c->gc.batch_counted) { snprintf(c->err, 512, "%s: the units of this batch are in the table already (a batch is counted once)", fn); return DG_ERR_ARG; }
    { const int rc = gc_ready(c, fn); if (rc) return rc; }
    if (c->n_reads) {
        const GcBatch b{c->reads_out.p, c->reports.p, c->cigfinal.p, (unsigned long long)c->used[0], (unsigned long long)c->used[1], c->n_reads, n_pair_mode, min_mapq};
        const int rc = gc_count_device(c, b, fn);
        if (rc) return rc;
    }
    c->gc.batch_counted = true;
    if (n_units) *n_units = (size_t)gc_units(c->n_reads, n_pair_mode);
    return DG_OK;
}

extern "C" int dg_gene_count_records(dg_ctx *c, int n_reads, int n_pair_mode, uint32_t min_mapq, const dg_read_out *reads, const dg_report_out *reports, size_t n_reports,
                                     const uint32_t *cigar, size_t n_ops, size_t *n_units)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_gene_count_records";
    if (n_units) *n_units = 0;
    if (n_reads < 0 || (n_reads && !reads) || (n_reports && !reports) || (n_ops && !cigar)) { snprintf(c->err, 512, "%s: %d reads, %zu reports and %zu CIGAR ops need their arrays", fn, n_reads, n_reports, n_ops); return DG_ERR_ARG; }
    { const int rc = gc_pair_mode_ok(c, fn, n_pair_mode, n_reads); if (rc) return rc; }
    const long long bad = gc_first_bad_read(reads, n_reads, reports, n_reports, n_ops);
    if (bad >= 0) { snprintf(c->err, 512, "%s: read %lld points outside the arrays (%zu reports, %zu CIGAR ops), or its best report is none of its own", fn, bad, n_reports, n_ops); return DG_ERR_ARG; }
    { const int rc = gc_ready(c, fn); if (rc) return rc; }
    if (!n_reads) return DG_OK;
    HIPCHK(c->gc.in_reads.ensure((size_t)n_reads)); HIPCHK(c->gc.in_rep.ensure(n_reports + 1)); HIPCHK(c->gc.in_cig.ensure(n_ops + 1));
    HIPCHK(hipMemcpyAsync(c->gc.in_reads.p, reads, (size_t)n_reads * sizeof(dg_read_out), hipMemcpyHostToDevice, c->stream));
    if (n_reports) HIPCHK(hipMemcpyAsync(c->gc.in_rep.p, reports, n_reports * sizeof(dg_report_out), hipMemcpyHostToDevice, c->stream));
    if (n_ops) HIPCHK(hipMemcpyAsync(c->gc.in_cig.p, cigar, n_ops * 4, hipMemcpyHostToDevice, c->stream));
    const GcBatch b{c->gc.in_reads.p, c->gc.in_rep.p, c->gc.in_cig.p, (unsigned long long)n_reports, (unsigned long long)n_ops, n_reads, n_pair_mode, min_mapq};
    { const int rc = gc_count_device(c, b, fn); if (rc) return rc; }
    HIPCHK(wait_stream(c));                          // (the caller's arrays are free again, and the staging buffers may take the next call's)
    if (n_units) *n_units = (size_t)gc_units(n_reads, n_pair_mode);
    return DG_OK;
}

extern "C" int dg_gene_add(dg_ctx *c, const uint64_t *counts, size_t n_rows)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_gene_add";
    { const int rc = gc_ready(c, fn); if (rc) return rc; }
    if (!counts || n_rows != c->gc.rows) { snprintf(c->err, 512, "%s: %zu rows, the table has %zu (4 + the annotation's genes)", fn, n_rows, c->gc.rows); return DG_ERR_ARG; }
    const size_t n = n_rows * 3;
    HIPCHK(c->gc.in.ensure(n));
    HIPCHK(hipMemcpyAsync(c->gc.in.p, counts, n * 8, hipMemcpyHostToDevice, c->stream));
    k_gc_add<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(c->gc.counts, c->gc.in.p, (unsigned long long)n);
    HIPCHK(hipGetLastError());
    HIPCHK(wait_stream(c));
    c->gc.nonempty = true;
    return DG_OK;
}

extern "C" int dg_gene_merge(dg_ctx *dst, dg_ctx *src)
{
    dg_ctx *c = dst;
    if (!dst || !src) return DG_ERR_ARG;
    const char *fn = "dg_gene_merge";
    if (dst == src || dst->device != src->device) { snprintf(c->err, 512, "%s: the two contexts must differ and be on one device", fn); return DG_ERR_ARG; }
    if (!src->gc.counts || !src->gc.nonempty) return DG_OK;
    { const int rc = gc_ready(dst, fn); if (rc) return rc; }
    if (dst->gc.gen != src->gc.gen || dst->gc.rows != src->gc.rows) {
        snprintf(c->err, 512, "%s: the tables were counted under different annotation generations (%llu and %llu)", fn, (unsigned long long)dst->gc.gen, (unsigned long long)src->gc.gen);
        return DG_ERR_ARG;
    }
    // behind everything the source's stream holds; the source's table is emptied on the destination's stream, which the call waits for
    HIPCHK(hipEventRecord(src->gc.ev[2], src->stream));
    HIPCHK(hipStreamWaitEvent(dst->stream, src->gc.ev[2], 0));
    const size_t n = dst->gc.rows * 3;
    k_gc_add<<<(unsigned)((n + 255) / 256), 256, 0, dst->stream>>>(dst->gc.counts, src->gc.counts, (unsigned long long)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(src->gc.counts, 0, n * 8, dst->stream));
    HIPCHK(wait_stream(dst));
    dst->gc.nonempty = true; src->gc.nonempty = false;
    return DG_OK;
}

extern "C" int dg_gene_reset(dg_ctx *c)
{
    if (!c) return DG_ERR_ARG;
    { const int rc = gc_ready(c, "dg_gene_reset", true); if (rc) return rc; }
    HIPCHK(wait_stream(c));
    return DG_OK;
}

extern "C" int dg_gene_download(dg_ctx *c, uint64_t *counts, size_t cap_rows)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_gene_download";
    if (!c->gc.counts) { const int rc = gc_ready(c, fn); if (rc) return rc; }
    if (!counts || cap_rows < c->gc.rows) { snprintf(c->err, 512, "%s: output capacity too small: %zu rows are needed", fn, c->gc.rows); return DG_ERR_CAPACITY; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(counts, c->gc.counts, c->gc.rows * 3 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));
    return DG_OK;
}

extern "C" int dg_gene_device(dg_ctx *c, void **counts)
{
    if (!c || !counts) return DG_ERR_ARG;
    if (!c->gc.counts) { const int rc = gc_ready(c, "dg_gene_device"); if (rc) return rc; }
    *counts = c->gc.counts;
    return DG_OK;
}

extern "C" int dg_gene_device_ms(dg_ctx *c, float *ms)
{
    if (!c || !ms) return DG_ERR_ARG;
    *ms = 0.f;
    if (!c->gc.timed) return DG_OK;
    HIPCHK(hipEventSynchronize(c->gc.ev[1]));
    HIPCHK(hipEventElapsedTime(ms, c->gc.ev[0], c->gc.ev[1]));
    return DG_OK;
}

// ------------------------------------------------------------------------------------------
// transcript-level expression (dg_txquant.h): the annotation's tables live with the index, a class table with every context
// ------------------------------------------------------------------------------------------
extern "C" int dg_tx_granules(int out[2])
{
    if (!out) return DG_ERR_ARG;
    out[0] = TX_THREADS; out[1] = TX_WAVE;
    return DG_OK;
}
extern "C" const char *dg_tx_word_name(int i) { return i >= 0 && i < 16 ? TX_WORD_NAMES[i] : nullptr; }

extern "C" int dg_tx_set_annotation(dg_ctx *c, const dg_rna_annot *a, size_t *n_exons_merged, size_t *n_segments)
{
    if (!c) return DG_ERR_ARG;
    if (n_exons_merged) *n_exons_merged = 0;
    if (n_segments) *n_segments = 0;
    IndexShared *sh = c->shared_ix;
    if (!sh || !a) { snprintf(c->err, 512, "dg_tx_set_annotation: no annotation (or a context without an index)"); return DG_ERR_ARG; }
    TxFlat fl;
    char why[400];
    if (!tx_flatten(c->ix.n_chr, a, fl, why, sizeof why)) { snprintf(c->err, 512, "dg_tx_set_annotation: %s", why); return DG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(sh->mu);
    void *d[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const void *src[6] = {fl.chr_first.data(), fl.seg_start.data(), fl.seg_ids.data(), fl.seg_off.data(), fl.tx.data(), fl.ex.data()};
    const size_t bytes[6] = {fl.chr_first.size() * 4, fl.seg_start.size() * 4, fl.seg_ids.size() * 4, fl.seg_off.size() * 8, fl.tx.size() * sizeof(TxTx), fl.ex.size() * sizeof(TxExon)};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 6 && e == hipSuccess; k++) {
        e = hipMalloc(&d[k], bytes[k] + 64);
        if (e == hipSuccess && bytes[k]) e = hipMemcpy(d[k], src[k], bytes[k], hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) { for (void *p : d) if (p) (void)hipFree(p); return fail(c, DG_ERR_HIP, "the expression stage's annotation tables", e); }
    // every call that reads the tables enqueues its kernels under sh->mu and waits for them there: the device is waited for, then the old ones are freed
    if (sh->tx_gen) { (void)hipDeviceSynchronize(); for (void *p : {(void *)sh->d_tx_chr_first, (void *)sh->d_tx_seg_start, (void *)sh->d_tx_seg_ids, (void *)sh->d_tx_seg_off, (void *)sh->d_tx_tx, (void *)sh->d_tx_ex}) (void)hipFree(p); }
    sh->d_tx_chr_first = (uint32_t *)d[0]; sh->d_tx_seg_start = (uint32_t *)d[1]; sh->d_tx_seg_ids = (uint32_t *)d[2]; sh->d_tx_seg_off = (uint64_t *)d[3]; sh->d_tx_tx = (TxTx *)d[4]; sh->d_tx_ex = (TxExon *)d[5];
    sh->tx_n_seg = fl.seg_start.size(); sh->tx_n_tx = a->n_tx; sh->tx_gen++;
    if (n_exons_merged) *n_exons_merged = fl.ex.size();
    if (n_segments) *n_segments = fl.seg_start.size();
    return DG_OK;
}

// the context's class table for the current annotation: made on first use; an empty one of another generation is replaced, a filled one is the caller's to reset
static int tx_ready(dg_ctx *c, const char *fn, bool fresh = false)
{
    IndexShared *sh = c->shared_ix;
    uint64_t gen = 0; uint32_t n_tx = 0;
    if (sh) { std::lock_guard<std::mutex> lk(sh->mu); gen = sh->tx_gen; n_tx = sh->tx_n_tx; }
    if (!gen) { snprintf(c->err, 512, "%s: no transcript annotation (dg_tx_set_annotation first)", fn); return DG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->tx.ready());
    HIPCHK(c->tx.words.ensure(8)); HIPCHK(c->tx.bw.ensure(8));
    if (c->tx.made && c->tx.gen == gen && !fresh) return DG_OK;
    if (c->tx.made && c->tx.gen != gen && c->tx.nonempty && !fresh) {
        snprintf(c->err, 512, "%s: the table holds classes of annotation generation %llu, the annotation is generation %llu now (dg_tx_reset first)", fn, (unsigned long long)c->tx.gen, (unsigned long long)gen);
        return DG_ERR_ARG;
    }
    HIPCHK(hipMemsetAsync(c->tx.words.p, 0, 64, c->stream));
    c->tx.tab[c->tx.cur].n_classes = 0; c->tx.tab[c->tx.cur].n_members = 0;
    c->tx.gen = gen; c->tx.n_tx = n_tx; c->tx.made = true; c->tx.nonempty = false; c->tx.fin_valid = false;
    return DG_OK;
}

#define TX_ENSURE(buf, n, what) do { if ((buf).ensure(n) != hipSuccess) { (void)hipGetLastError(); \
    snprintf(c->err, 512, "%s: not enough device memory: %s need %zu bytes", fn, what, (size_t)(n) * sizeof(*(buf).p)); return DG_ERR_CAPACITY; } } while (0)

// everything a build of n items sorts and scans in
static int tx_build_bufs(dg_ctx *c, const char *fn, size_t n)
{
    TxState &x = c->tx;
    for (int k = 0; k < 2; k++) { TX_ENSURE(x.sort.k[k], n, "the sorter's keys"); TX_ENSURE(x.sort.v[k], n, "the sorter's values"); }
    if (x.sort.ensure((uint32_t)n) != hipSuccess) { (void)hipGetLastError(); snprintf(c->err, 512, "%s: not enough device memory: %s need %zu bytes", fn, x.sort.short_of, x.sort.short_bytes); return DG_ERR_CAPACITY; }
    TX_ENSURE(x.head, n, "the heads"); TX_ENSURE(x.sz, n, "the heads' sizes"); TX_ENSURE(x.sz_ex, n, "the heads' offsets");
    TX_ENSURE(x.scan_sums, (n + SCAN_TILE - 1) / SCAN_TILE + 1, "the scan's sums");
    return DG_OK;
}

// The class building: the table's classes and the items b (a batch's pool, another table, a downloaded table) sorted by their lists' hashes, equal lists
// made one class, into the context's other table; on success the two change places.  b_members: the ids b holds; b_keys_ready: the sorter's first key
// buffer holds b's keys already, behind the table's.  The call waits for the stream.
static int tx_build(dg_ctx *c, const char *fn, TxItems b, uint64_t b_members, bool b_keys_ready)
{
    TxState &x = c->tx;
    TxTab &A = x.tab[x.cur], &O = x.tab[x.cur ^ 1];
    if (!b.n) return DG_OK;
    const TxTwo s{TxItems{A.off.p, A.ids.p, A.cnt.p, (uint64_t)A.n_classes}, b};
    const uint64_t n = (uint64_t)A.n_classes + b.n, members_in = (uint64_t)A.n_members + b_members;
    if (n >= 0xFFFFFFF0ull || members_in >= 0xFFFFFFF0ull) { snprintf(c->err, 512, "%s: %llu items with %llu ids are more than one class table takes", fn, (unsigned long long)n, (unsigned long long)members_in); return DG_ERR_RANGE; }
    { const int rc = tx_build_bufs(c, fn, (size_t)n); if (rc) return rc; }
    const unsigned grid = (unsigned)((n + 255) / 256);
    HIPCHK(hipEventRecord(x.ev[2], c->stream));
    k_tx_hash<<<grid, 256, 0, c->stream>>>(s, n, b_keys_ready ? (unsigned long long)A.n_classes : n, tx_hash_mask(x.hash_bits), x.sort.k[0].p, x.sort.v[0].p);
    int which = 0;
    { const int rc = x.sort.sort(c, (uint32_t)n, (x.hash_bits + 3) / 4 * 4, which); if (rc) return rc; }
    HIPCHK(hipMemsetAsync(x.bst.d, 0, 4 * sizeof(uint32_t), c->stream));
    k_tx_heads<<<grid, 256, 0, c->stream>>>(s, n, x.sort.k[which].p, x.sort.v[which].p, x.head.p, x.sz.p, x.bst.d);
    rs_scan_u32(c->stream, x.head.p, x.head.p, (uint32_t)n, x.scan_sums.p, x.bst.d);
    rs_scan_u32(c->stream, x.sz.p, x.sz_ex.p, (uint32_t)n, x.scan_sums.p, x.bst.d + 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(x.ev[3], c->stream));
    HIPCHK(x.bst.fetch(c->stream));
    HIPCHK(wait_stream(c));
    x.ms[1] += x.ev.ms(2, 3);
    if (x.bst.h[2]) {
        // two lists under one hash: their items may interleave in the sorted order, so runs are not classes.  This build is finished on the host, exactly.
        std::vector<uint64_t> off[2], cnt[2]; std::vector<uint32_t> ids[2];
        const TxItems *src[2] = {&s.a, &s.b};
        TxTwo hs;
        TxItems *dst[2] = {&hs.a, &hs.b};
        for (int k = 0; k < 2; k++) {
            const TxItems &q = *src[k];
            off[k].assign((size_t)q.n + 1, 0ull);
            if (q.n) HIPCHK(hipMemcpy(off[k].data(), q.off, ((size_t)q.n + 1) * 8, hipMemcpyDeviceToHost));
            const uint64_t base = off[k][0], m = off[k][(size_t)q.n] - base;
            for (uint64_t &o : off[k]) o -= base;
            ids[k].resize((size_t)m);
            if (m) HIPCHK(hipMemcpy(ids[k].data(), q.ids + base, (size_t)m * 4, hipMemcpyDeviceToHost));
            if (q.cnt && q.n) { cnt[k].resize((size_t)q.n); HIPCHK(hipMemcpy(cnt[k].data(), q.cnt, (size_t)q.n * 8, hipMemcpyDeviceToHost)); }
            *dst[k] = TxItems{off[k].data(), ids[k].data(), q.cnt && q.n ? cnt[k].data() : nullptr, q.n};
        }
        TxHostTab t;
        tx_build_host(hs, t);
        TX_ENSURE(O.off, t.off.size(), "the class table's offsets"); TX_ENSURE(O.ids, t.ids.size(), "the class table's ids"); TX_ENSURE(O.cnt, t.cnt.size(), "the class table's counts");
        HIPCHK(hipMemcpy(O.off.p, t.off.data(), t.off.size() * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(O.ids.p, t.ids.data(), t.ids.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(O.cnt.p, t.cnt.data(), t.cnt.size() * 8, hipMemcpyHostToDevice));
        O.n_classes = t.cnt.size(); O.n_members = t.ids.size();
    } else {
        const size_t nc = x.bst.h[0], nm = x.bst.h[1];
        TX_ENSURE(O.off, nc + 1, "the class table's offsets"); TX_ENSURE(O.ids, nm, "the class table's ids"); TX_ENSURE(O.cnt, nc, "the class table's counts");
        HIPCHK(hipMemsetAsync(O.cnt.p, 0, nc * 8, c->stream));
        HIPCHK(hipEventRecord(x.ev[2], c->stream));
        k_tx_csr<<<grid, 256, 0, c->stream>>>(s, n, x.sort.v[which].p, x.sz.p, x.head.p, x.sz_ex.p, (unsigned long long)nc, (unsigned long long)nm, O.off.p, O.ids.p, (unsigned long long *)O.cnt.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(x.ev[3], c->stream));
        HIPCHK(wait_stream(c));
        x.ms[1] += x.ev.ms(2, 3);
        O.n_classes = nc; O.n_members = nm;
    }
    x.cur ^= 1;
    return DG_OK;
}

// the compatibility passes over the records b holds in HBM and the build that folds the batch's classes in
static int tx_count_device(dg_ctx *c, GcBatch b, uint32_t strand_mode, const char *fn)
{
    IndexShared *sh = c->shared_ix;
    TxState &x = c->tx;
    const unsigned long long n_units = gc_units(b.n_reads, b.n_pair_mode);
    const unsigned long long n_wg = (n_units + TX_THREADS - 1) / TX_THREADS;
    if (!n_units) return DG_OK;
    if (n_wg > 0x7FFFFFFFull) { snprintf(c->err, 512, "%s: %llu units are more than one call takes", fn, n_units); return DG_ERR_ARG; }
    TX_ENSURE(x.size, (size_t)n_units, "the units' sizes"); TX_ENSURE(x.hash, (size_t)n_units, "the units' hashes");
    TX_ENSURE(x.wg, (size_t)n_wg * 8, "the workgroups' lines"); TX_ENSURE(x.tile_sz, (size_t)n_wg, "the workgroups' sums"); TX_ENSURE(x.tile_items, (size_t)n_wg, "the workgroups' sums");
    const uint64_t mask = tx_hash_mask(x.hash_bits);
    x.ms[0] = x.ms[1] = 0.f;
    {   // the tables are read and the kernels that use them enqueued under the index's lock: dg_tx_set_annotation replaces them under the same lock and waits
        // for the device before it frees the old ones.  The lock is not held across the waits below, so the clones of an index count side by side
        std::lock_guard<std::mutex> lk(sh->mu);
        if (sh->tx_gen != x.gen) { snprintf(c->err, 512, "%s: the annotation was replaced while the call was being prepared", fn); return DG_ERR_ARG; }
        const TxTable T{sh->d_tx_chr_first, sh->d_tx_seg_start, sh->d_tx_seg_off, sh->d_tx_seg_ids, sh->d_tx_tx, sh->d_tx_ex, c->ix.n_chr, sh->tx_n_tx};
        HIPCHK(hipEventRecord(x.ev[0], c->stream));
        k_tx_count<<<(unsigned)n_wg, TX_THREADS, 0, c->stream>>>(b, T, n_units, strand_mode, mask, x.size.p, x.hash.p, x.wg.p, x.tile_sz.p, x.tile_items.p);
        k_tx_top<<<1, WG_THREADS, 0, c->stream>>>(x.wg.p, (uint32_t)n_wg, x.bw.p, x.tile_sz.p, x.tile_items.p, x.pst.d);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(x.ev[1], c->stream));
    }
    HIPCHK(x.pst.fetch(c->stream));
    HIPCHK(wait_stream(c));
    x.ms[0] += x.ev.ms(0, 1);
    const unsigned long long n_ids = x.pst.h[0], n_items = x.pst.h[1];
    if (n_items) {
        const size_t n_tab = x.tab[x.cur].n_classes;
        if (n_tab + n_items >= 0xFFFFFFF0ull || n_ids >= 0xFFFFFFF0ull) { snprintf(c->err, 512, "%s: %llu items with %llu ids are more than one class table takes", fn, n_tab + n_items, n_ids); return DG_ERR_RANGE; }
        { const int rc = tx_build_bufs(c, fn, n_tab + (size_t)n_items); if (rc) return rc; }
        TX_ENSURE(x.pool_off, (size_t)n_items + 1, "the pool's offsets"); TX_ENSURE(x.pool_ids, (size_t)n_ids, "the pool's ids");
        {
            std::lock_guard<std::mutex> lk(sh->mu);
            if (sh->tx_gen != x.gen) { snprintf(c->err, 512, "%s: the annotation was replaced while the call was running", fn); return DG_ERR_ARG; }
            const TxTable T{sh->d_tx_chr_first, sh->d_tx_seg_start, sh->d_tx_seg_off, sh->d_tx_seg_ids, sh->d_tx_tx, sh->d_tx_ex, c->ix.n_chr, sh->tx_n_tx};
            HIPCHK(hipEventRecord(x.ev[0], c->stream));
            k_tx_write<<<(unsigned)n_wg, TX_THREADS, 0, c->stream>>>(b, T, n_units, strand_mode, x.size.p, x.hash.p, x.tile_sz.p, x.tile_items.p, n_items, n_ids, x.pool_off.p, x.pool_ids.p, x.sort.k[0].p + n_tab);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(x.ev[1], c->stream));
        }
        HIPCHK(wait_stream(c));
        x.ms[0] += x.ev.ms(0, 1);
        const int rc = tx_build(c, fn, TxItems{x.pool_off.p, x.pool_ids.p, nullptr, n_items}, n_ids, true);
        if (rc) return rc;
    }
    k_gc_add<<<1, 256, 0, c->stream>>>(x.words.p, x.bw.p, 8ull);
    HIPCHK(hipGetLastError());
    HIPCHK(wait_stream(c));
    x.timed = true; x.nonempty = true; x.fin_valid = false; x.strand_mode = strand_mode;
    return DG_OK;
}

extern "C" int dg_batch_accumulate_tx(dg_ctx *c, int n_pair_mode, uint32_t min_mapq, uint32_t strand_mode, size_t *n_units)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_batch_accumulate_tx";
    if (n_units) *n_units = 0;
    { IndexShared *sh = c->shared_ix; uint64_t gen = 0; if (sh) { std::lock_guard<std::mutex> lk(sh->mu); gen = sh->tx_gen; }
      if (!gen) { snprintf(c->err, 512, "%s: no transcript annotation (dg_tx_set_annotation first)", fn); return DG_ERR_ARG; } }
    if (!c->batch_done) { snprintf(c->err, 512, "%s: the context has no finished batch (upload and run one first)", fn); return DG_ERR_ARG; }
    { const int rc = gc_pair_mode_ok(c, fn, n_pair_mode, c->n_reads); if (rc) return rc; }
    if (strand_mode > 2u) { snprintf(c->err, 512, "%s: strand_mode %u is none of 0, 1, 2", fn, strand_mode); return DG_ERR_ARG; }
    if (c->n_reads && !c->full_valid) { snprintf(c->err, 512, "%s: the last batch has no full records (it was mapped through dg_map_batch_compact)", fn); return DG_ERR_ARG; }
    if (c->tx.batch_counted) { snprintf(c->err, 512, "%s: the units of this batch are in the table already (a batch is counted once)", fn); return DG_ERR_ARG; }
    { const int rc = tx_ready(c, fn); if (rc) return rc; }
    if (c->n_reads) {
        const GcBatch b{c->reads_out.p, c->reports.p, c->cigfinal.p, (unsigned long long)c->used[0], (unsigned long long)c->used[1], c->n_reads, n_pair_mode, min_mapq};
        const int rc = tx_count_device(c, b, strand_mode, fn);
        if (rc) return rc;
    }
    c->tx.batch_counted = true;
    if (n_units) *n_units = (size_t)gc_units(c->n_reads, n_pair_mode);
    return DG_OK;
}

extern "C" int dg_tx_count_records(dg_ctx *c, int n_reads, int n_pair_mode, uint32_t min_mapq, uint32_t strand_mode, const dg_read_out *reads, const dg_report_out *reports, size_t n_reports,
                                   const uint32_t *cigar, size_t n_ops, size_t *n_units)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_tx_count_records";
    if (n_units) *n_units = 0;
    if (n_reads < 0 || (n_reads && !reads) || (n_reports && !reports) || (n_ops && !cigar)) { snprintf(c->err, 512, "%s: %d reads, %zu reports and %zu CIGAR ops need their arrays", fn, n_reads, n_reports, n_ops); return DG_ERR_ARG; }
    { const int rc = gc_pair_mode_ok(c, fn, n_pair_mode, n_reads); if (rc) return rc; }
    if (strand_mode > 2u) { snprintf(c->err, 512, "%s: strand_mode %u is none of 0, 1, 2", fn, strand_mode); return DG_ERR_ARG; }
    const long long bad = gc_first_bad_read(reads, n_reads, reports, n_reports, n_ops);
    if (bad >= 0) { snprintf(c->err, 512, "%s: read %lld points outside the arrays (%zu reports, %zu CIGAR ops), or its best report is none of its own", fn, bad, n_reports, n_ops); return DG_ERR_ARG; }
    { const int rc = tx_ready(c, fn); if (rc) return rc; }
    if (!n_reads) return DG_OK;
    HIPCHK(c->tx.in_reads.ensure((size_t)n_reads)); HIPCHK(c->tx.in_rep.ensure(n_reports + 1)); HIPCHK(c->tx.in_cig.ensure(n_ops + 1));
    HIPCHK(hipMemcpyAsync(c->tx.in_reads.p, reads, (size_t)n_reads * sizeof(dg_read_out), hipMemcpyHostToDevice, c->stream));
    if (n_reports) HIPCHK(hipMemcpyAsync(c->tx.in_rep.p, reports, n_reports * sizeof(dg_report_out), hipMemcpyHostToDevice, c->stream));
    if (n_ops) HIPCHK(hipMemcpyAsync(c->tx.in_cig.p, cigar, n_ops * 4, hipMemcpyHostToDevice, c->stream));
    const GcBatch b{c->tx.in_reads.p, c->tx.in_rep.p, c->tx.in_cig.p, (unsigned long long)n_reports, (unsigned long long)n_ops, n_reads, n_pair_mode, min_mapq};
    { const int rc = tx_count_device(c, b, strand_mode, fn); if (rc) return rc; }
    if (n_units) *n_units = (size_t)gc_units(n_reads, n_pair_mode);
    return DG_OK;
}

extern "C" int dg_tx_add(dg_ctx *c, const uint64_t *off, const uint32_t *ids, const uint64_t *count, size_t n_classes, const uint64_t *words8)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_tx_add";
    { const int rc = tx_ready(c, fn); if (rc) return rc; }
    TxState &x = c->tx;
    if (!words8) { snprintf(c->err, 512, "%s: the table's eight words are missing", fn); return DG_ERR_ARG; }
    size_t where = 0;
    const char *what = tx_bad_table(off, ids, count, n_classes, x.n_tx, where);
    if (what) { snprintf(c->err, 512, "%s: class %zu: %s (%u transcripts)", fn, where, what, x.n_tx); return DG_ERR_ARG; }
    const size_t n_members = n_classes ? (size_t)off[n_classes] : 0;
    TX_ENSURE(x.in_words, 8, "the words");
    if (n_classes) {
        TX_ENSURE(x.in_off, n_classes + 1, "the added table's offsets"); TX_ENSURE(x.in_ids, n_members, "the added table's ids"); TX_ENSURE(x.in_cnt, n_classes, "the added table's counts");
        HIPCHK(hipMemcpyAsync(x.in_off.p, off, (n_classes + 1) * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(x.in_ids.p, ids, n_members * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(x.in_cnt.p, count, n_classes * 8, hipMemcpyHostToDevice, c->stream));
        x.ms[1] = 0.f;
        const int rc = tx_build(c, fn, TxItems{x.in_off.p, x.in_ids.p, x.in_cnt.p, (uint64_t)n_classes}, n_members, false);
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(x.in_words.p, words8, 64, hipMemcpyHostToDevice, c->stream));
    k_gc_add<<<1, 256, 0, c->stream>>>(x.words.p, x.in_words.p, 8ull);
    HIPCHK(hipGetLastError());
    HIPCHK(wait_stream(c));
    x.nonempty = true; x.fin_valid = false;
    return DG_OK;
}

extern "C" int dg_tx_merge(dg_ctx *dst, dg_ctx *src)
{
    dg_ctx *c = dst;
    if (!dst || !src) return DG_ERR_ARG;
    const char *fn = "dg_tx_merge";
    if (dst == src || dst->device != src->device) { snprintf(c->err, 512, "%s: the two contexts must differ and be on one device", fn); return DG_ERR_ARG; }
    if (!src->tx.made || !src->tx.nonempty) return DG_OK;
    { const int rc = tx_ready(dst, fn); if (rc) return rc; }
    if (dst->tx.gen != src->tx.gen) {
        snprintf(c->err, 512, "%s: the tables were built under different annotation generations (%llu and %llu)", fn, (unsigned long long)dst->tx.gen, (unsigned long long)src->tx.gen);
        return DG_ERR_ARG;
    }
    // behind everything the source's stream holds; the source's table is emptied on the destination's stream, which the call waits for
    HIPCHK(hipEventRecord(src->tx.ev[6], src->stream));
    HIPCHK(hipStreamWaitEvent(dst->stream, src->tx.ev[6], 0));
    const TxTab &S = src->tx.tab[src->tx.cur];
    dst->tx.ms[1] = 0.f;
    { const int rc = tx_build(dst, fn, TxItems{S.off.p, S.ids.p, S.cnt.p, (uint64_t)S.n_classes}, S.n_members, false); if (rc) return rc; }
    k_gc_add<<<1, 256, 0, dst->stream>>>(dst->tx.words.p, src->tx.words.p, 8ull);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(src->tx.words.p, 0, 64, dst->stream));
    HIPCHK(wait_stream(dst));
    src->tx.tab[src->tx.cur].n_classes = 0; src->tx.tab[src->tx.cur].n_members = 0;
    if (!dst->tx.nonempty) dst->tx.strand_mode = src->tx.strand_mode;
    dst->tx.nonempty = true; dst->tx.fin_valid = false; src->tx.nonempty = false; src->tx.fin_valid = false;
    return DG_OK;
}

extern "C" int dg_tx_reset(dg_ctx *c)
{
    if (!c) return DG_ERR_ARG;
    { const int rc = tx_ready(c, "dg_tx_reset", true); if (rc) return rc; }
    HIPCHK(wait_stream(c));
    return DG_OK;
}

extern "C" int dg_tx_classes_size(dg_ctx *c, size_t *n_classes, size_t *n_members)
{
    if (!c) return DG_ERR_ARG;
    if (n_classes) *n_classes = 0;
    if (n_members) *n_members = 0;
    if (!c->tx.made) { const int rc = tx_ready(c, "dg_tx_classes_size"); if (rc) return rc; }
    if (n_classes) *n_classes = c->tx.tab[c->tx.cur].n_classes;
    if (n_members) *n_members = c->tx.tab[c->tx.cur].n_members;
    return DG_OK;
}

extern "C" int dg_tx_classes_download(dg_ctx *c, uint64_t *off, uint32_t *ids, uint64_t *count, size_t cap_classes, size_t cap_members, uint64_t *words8)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_tx_classes_download";
    if (!c->tx.made) { const int rc = tx_ready(c, fn); if (rc) return rc; }
    const TxTab &A = c->tx.tab[c->tx.cur];
    if (!off || !words8 || cap_classes < A.n_classes || cap_members < A.n_members || (A.n_classes && (!ids || !count))) {
        snprintf(c->err, 512, "%s: output capacity too small: %zu classes and %zu ids are needed", fn, A.n_classes, A.n_members); return DG_ERR_CAPACITY;
    }
    HIPCHK(hipSetDevice(c->device));
    off[0] = 0;
    if (A.n_classes) {
        HIPCHK(hipMemcpyAsync(off, A.off.p, (A.n_classes + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(ids, A.ids.p, A.n_members * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(count, A.cnt.p, A.n_classes * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipMemcpyAsync(words8, c->tx.words.p, 64, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));
    return DG_OK;
}

extern "C" int dg_tx_finish(dg_ctx *c, uint32_t flags, uint64_t frag_mean, uint32_t max_rounds, size_t *n_words, float *device_ms)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_tx_finish";
    if (n_words) *n_words = 0;
    if (device_ms) *device_ms = 0.f;
    if (flags) { snprintf(c->err, 512, "%s: flags 0x%x: no flag is defined", fn, flags); return DG_ERR_ARG; }
    { const int rc = tx_ready(c, fn); if (rc) return rc; }
    TxState &x = c->tx;
    IndexShared *sh = c->shared_ix;
    const TxTab &A = x.tab[x.cur];
    const uint32_t n_tx = x.n_tx, n_wg = (n_tx + 255u) / 256u;
    const unsigned long long nc = A.n_classes, nm = A.n_members;
    x.fin_valid = false;
    TX_ENSURE(x.S, n_tx, "S"); TX_ENSURE(x.S2, n_tx, "S'"); TX_ENSURE(x.theta, n_tx, "theta"); TX_ENSURE(x.active, n_tx, "the active marks"); TX_ENSURE(x.eff, n_tx, "the effective lengths");
    TX_ENSURE(x.conv, n_wg, "the convergence words"); TX_ENSURE(x.res, (size_t)n_tx + 16, "the result words");
    HIPCHK(hipEventRecord(x.ev[4], c->stream));
    HIPCHK(hipMemsetAsync(x.active.p, 0, (size_t)n_tx * 4, c->stream));
    if (nm) k_tx_active<<<(unsigned)((nm + 255) / 256), 256, 0, c->stream>>>(A.ids.p, nm, n_tx, x.active.p);
    k_tx_em_prep<<<1, WG_THREADS, 0, c->stream>>>(x.active.p, n_tx, (const unsigned long long *)A.cnt.p, nc, x.pst.d);
    HIPCHK(hipGetLastError());
    HIPCHK(x.pst.fetch(c->stream));
    HIPCHK(hipMemcpyAsync(x.wst.h, x.words.p, 64, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));
    const unsigned long long M = x.pst.h[0], N = x.pst.h[1];
    if (N >= TX_MAX_N) { snprintf(c->err, 512, "%s: the counts sum to %llu, the EM takes less than 2^33", fn, N); return DG_ERR_RANGE; }
    const unsigned long long *w = x.wst.h;
    const unsigned long long mean = w[TXW_FL_N] ? w[TXW_FL_SUM] / w[TXW_FL_N] : (unsigned long long)frag_mean;
    {   // the transcripts' lengths are read under the index's lock (dg_tx_set_annotation waits for the device before it frees them)
        std::lock_guard<std::mutex> lk(sh->mu);
        if (sh->tx_gen != x.gen) { snprintf(c->err, 512, "%s: the annotation was replaced while the call was being prepared", fn); return DG_ERR_ARG; }
        k_tx_start<<<n_wg, 256, 0, c->stream>>>(sh->d_tx_tx, n_tx, x.active.p, M ? N * TX_F / M : 0ull, mean, x.S.p, x.S2.p, x.eff.p, x.theta.p);
        HIPCHK(hipGetLastError());
    }
    unsigned long long rounds = 0, converged = M ? 0ull : 1ull;
    while (M && rounds < max_rounds) {
        if (nc) k_tx_em<<<(unsigned)((nc + 255) / 256), 256, 0, c->stream>>>(A.off.p, A.ids.p, (const unsigned long long *)A.cnt.p, nc, x.theta.p, x.S2.p);
        k_tx_theta<<<n_wg, 256, 0, c->stream>>>(n_tx, x.eff.p, x.S.p, x.S2.p, x.theta.p, x.conv.p);
        rounds++;
        if (rounds == max_rounds || rounds % TX_CHECK_EVERY == 0) {       // (the rounds between two looks are enqueued without a wait)
            k_tx_conv<<<1, WG_THREADS, 0, c->stream>>>(x.conv.p, n_wg, x.pst.d);
            HIPCHK(hipGetLastError());
            HIPCHK(x.pst.fetch(c->stream));
            HIPCHK(wait_stream(c));
            converged = x.pst.h[2] ? 0ull : 1ull;
            if (converged && rounds % TX_CHECK_EVERY == 0) break;
        }
    }
    const unsigned long long tail[16] = {w[0], w[1], w[2], w[3], w[4], nc, nm, M, rounds, converged, w[TXW_FL_SUM], w[TXW_FL_N], mean, x.strand_mode, 0ull, 0ull};
    HIPCHK(hipMemcpyAsync(x.res.p, x.S.p, (size_t)n_tx * 8, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(x.res.p + n_tx, tail, sizeof tail, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(x.ev[5], c->stream));
    HIPCHK(wait_stream(c));
    x.ms[2] = x.ev.ms(4, 5);
    x.n_words = (size_t)n_tx + 16; x.fin_valid = true;
    if (n_words) *n_words = x.n_words;
    if (device_ms) *device_ms = x.ms[2];
    return DG_OK;
}

extern "C" int dg_tx_download(dg_ctx *c, uint64_t *words, size_t cap_words)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_tx_download";
    if (!c->tx.fin_valid) { snprintf(c->err, 512, "%s: no result (dg_tx_finish first, and no table call behind it)", fn); return DG_ERR_ARG; }
    if (!words || cap_words < c->tx.n_words) { snprintf(c->err, 512, "%s: output capacity too small: %zu words are needed", fn, c->tx.n_words); return DG_ERR_CAPACITY; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(words, c->tx.res.p, c->tx.n_words * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));
    return DG_OK;
}

extern "C" int dg_tx_device(dg_ctx *c, void **words, size_t *n_words)
{
    if (!c || !words || !n_words) return DG_ERR_ARG;
    if (!c->tx.fin_valid) { snprintf(c->err, 512, "dg_tx_device: no result (dg_tx_finish first, and no table call behind it)"); return DG_ERR_ARG; }
    *words = c->tx.res.p; *n_words = c->tx.n_words;
    return DG_OK;
}

extern "C" int dg_tx_device_ms(dg_ctx *c, float ms[3])
{
    if (!c || !ms) return DG_ERR_ARG;
    for (int k = 0; k < 3; k++) ms[k] = c->tx.ms[k];
    return DG_OK;
}

extern "C" int dg_tx_format(const uint64_t *words, size_t n_words, const dg_rna_annot *a, const char *const *names, char *out, size_t cap, size_t *n_bytes)
{
    if (n_bytes) *n_bytes = 0;
    if (!words || !a || !a->tx || !names || n_words != (size_t)a->n_tx + 16 || (!out && cap)) return DG_ERR_ARG;
    char why[400];
    if (!rm_validate(1 << 30, a, why, sizeof why)) return DG_ERR_ARG;
    std::vector<uint32_t> len(a->n_tx);
    std::vector<dg_rna_exon> m;
    for (uint32_t t = 0; t < a->n_tx; t++) { tx_merge_exons(a, a->tx[t], m); uint32_t L = 0; for (const dg_rna_exon &e : m) L += e.end - e.start; len[t] = L; }
    const std::string text = tx_format(words, a->n_tx, len.data(), names);
    if (n_bytes) *n_bytes = text.size();
    if (cap < text.size()) return DG_ERR_CAPACITY;
    if (!text.empty()) memcpy(out, text.data(), text.size());
    return DG_OK;
}

// ------------------------------------------------------------------------------------------
// the coverage track of the sorted array (dg_coverage.h): built in HBM from the sorted records and their places, in buffers of its own
// ------------------------------------------------------------------------------------------
extern "C" int dg_bam_coverage_granules(int out[2])
{
    if (!out) return DG_ERR_ARG;
    out[0] = CV_THREADS; out[1] = RS_TILE;
    return DG_OK;
}

extern "C" int dg_bam_coverage_finish(dg_ctx *c, uint32_t flags, uint32_t exclude_flags, uint32_t min_mapq, size_t *n_entries, size_t *n_bytes, uint64_t stats[7], float *device_ms)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_bam_coverage_finish";
    if (n_entries) *n_entries = 0;
    if (n_bytes) *n_bytes = 0;
    if (device_ms) *device_ms = 0.f;
    if (stats) for (int k = 0; k < 7; k++) stats[k] = 0;
    c->cv.valid = false; c->cv.n_entries = 0; c->cv.bytes = 0; c->cv.passes = 0;
    for (float &m : c->cv.ms) m = 0.f;
    BsView sv;
    { const int rc = bs_view(c, fn, sv); if (rc) return rc; }
    if (flags & ~(DG_COV_ENTRIES_ONLY | DG_COV_STRAND_PLUS | DG_COV_STRAND_MINUS)) { snprintf(c->err, 512, "%s: flags 0x%x hold a bit that is none of DG_COV_ENTRIES_ONLY, DG_COV_STRAND_PLUS, DG_COV_STRAND_MINUS", fn, flags); return DG_ERR_ARG; }
    const bool text = !(flags & DG_COV_ENTRIES_ONLY);
    IndexShared *sh = c->shared_ix;
    if (text && (!sh || !sh->chr_names_set)) { snprintf(c->err, 512, "%s: the chromosome names are missing (dg_set_chr_names), and DG_COV_ENTRIES_ONLY is not set", fn); return DG_ERR_ARG; }
    HIPCHK(c->cv.ready());
    const size_t n = sv.n, n_raw = sv.n_raw;
    const int n_chr = sv.n_chr;
    if (n_chr < 1) { snprintf(c->err, 512, "%s: %d chromosomes", fn, n_chr); return DG_ERR_ARG; }
    if (!n) { c->cv.valid = true; return DG_OK; }
    const CvFilter f{flags, exclude_flags, min_mapq};
    const uint32_t tiles = (uint32_t)((n + CV_THREADS - 1) / CV_THREADS);
    BS_ENSURE(c->cv.blk_off, n, "the records' block offsets"); BS_ENSURE(c->cv.blk_tile, (size_t)tiles + 1, "the per-workgroup block counts");
    BS_ENSURE(c->cv.part, (size_t)CV_PLANES * tiles, "the per-workgroup values");
    HIPCHK(hipMemsetAsync(c->cv.stat.d, 0, CV_ST_WORDS * 8, c->stream));
    HIPCHK(hipEventRecord(c->cv.ev[0], c->stream));
    k_cv_count<<<tiles, CV_THREADS, 0, c->stream>>>(sv.rec, sv.dst_off, sv.tile, (uint32_t)n, (unsigned long long)n_raw, n_chr, f, c->cv.blk_off.p, c->cv.blk_tile.p, c->cv.part.p);
    k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->cv.blk_tile.p, tiles, c->cv.stat.d + CV_ST_BLOCKS, c->cv.part.p, 5, 2, c->cv.stat.d + CV_ST_COUNTED);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->cv.ev[1], c->stream));
    HIPCHK(c->cv.stat.fetch(c->stream));
    HIPCHK(wait_stream(c));                                       // the first wait: how many events, which digits their keys differ in, and what was out of range
    if (c->cv.stat.h[CV_ST_NBAD]) {
        snprintf(c->err, 512, "%s: record %llu of the sorted array has a block that ends behind position 2^32 - 1: an entry cannot hold it; no track was built", fn, ~c->cv.stat.h[CV_ST_NBAD]);
        return DG_ERR_RANGE;
    }
    const unsigned long long n_blocks = c->cv.stat.h[CV_ST_BLOCKS], n_counted = c->cv.stat.h[CV_ST_COUNTED], aligned = c->cv.stat.h[CV_ST_ALIGNED];
    if (2 * n_blocks >= 0xFFFFF000ull) { snprintf(c->err, 512, "%s: %llu events (two per block) are more than the sorter takes (2^32 - 1, less a tile)", fn, 2 * n_blocks); return DG_ERR_CAPACITY; }
    c->cv.ms[0] = c->cv.ev.ms(0, 1);
    auto done = [&](size_t ne, size_t nb, unsigned long long n_bp, unsigned long long covered, unsigned long long deepest) {
        float total = 0.f;
        for (float m : c->cv.ms) total += m;
        c->cv.valid = true; c->cv.n_entries = ne; c->cv.bytes = nb;
        if (n_entries) *n_entries = ne;
        if (n_bytes) *n_bytes = nb;
        if (device_ms) *device_ms = total;
        if (stats) { stats[0] = n_counted; stats[1] = n_blocks; stats[2] = n_bp; stats[3] = ne; stats[4] = covered; stats[5] = aligned; stats[6] = deepest; }
        return DG_OK;
    };
    if (!n_blocks) return done(0, 0, 0, 0, 0);
    const uint32_t n_ev = (uint32_t)(2 * n_blocks), etiles = (n_ev + CV_THREADS - 1) / CV_THREADS;
    for (int k = 0; k < 2; k++) { BS_ENSURE(c->cv.sort.k[k], (size_t)n_ev, "the events' keys"); BS_ENSURE(c->cv.sort.v[k], (size_t)n_ev, "the events' deltas"); }
    BS_ENSURE_SORT(c->cv.sort, n_ev);
    BS_ENSURE(c->cv.incl, (size_t)n_ev, "the scanned deltas"); BS_ENSURE(c->cv.mark, (size_t)n_ev, "the events' marks");
    BS_ENSURE(c->cv.dep_tile, (size_t)etiles + 1, "the per-workgroup depth sums"); BS_ENSURE(c->cv.tile_last, (size_t)etiles + 1, "the per-workgroup last tails");
    BS_ENSURE(c->cv.tile_prev, (size_t)etiles + 1, "the per-workgroup previous tails"); BS_ENSURE(c->cv.cnt_tile, (size_t)etiles + 1, "the per-workgroup breakpoint counts");
    BS_ENSURE(c->cv.part, (size_t)etiles, "the per-workgroup values");
    const int bits = std::min(cv_key_bits(~c->cv.stat.h[CV_ST_NMIN], c->cv.stat.h[CV_ST_MAX]), cv_key_bits_max(n_chr));
    int which = 0;
    HIPCHK(hipEventRecord(c->cv.ev[2], c->stream));
    k_cv_emit<<<tiles, CV_THREADS, 0, c->stream>>>(sv.rec, sv.dst_off, sv.tile, (uint32_t)n, (unsigned long long)n_raw, n_chr, f, c->cv.blk_off.p, c->cv.blk_tile.p, n_blocks, c->cv.sort.k[0].p, c->cv.sort.v[0].p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->cv.ev[3], c->stream));
    {
        const int rc = c->cv.sort.sort(c, n_ev, bits, which);
        if (rc) return rc;
        c->cv.passes = (bits + 3) / 4;
    }
    HIPCHK(hipEventRecord(c->cv.ev[4], c->stream));
    const uint64_t *skey = c->cv.sort.k[which].p;
    k_cv_depth<<<etiles, CV_THREADS, 0, c->stream>>>(c->cv.sort.v[which].p, n_ev, c->cv.incl.p, c->cv.dep_tile.p);
    k_tiles_top<uint32_t><<<1, 256, 0, c->stream>>>(c->cv.dep_tile.p, etiles, (uint32_t *)(c->cv.stat.d + CV_ST_DEPTH_END));
    k_cv_tails<<<etiles, CV_THREADS, 0, c->stream>>>(skey, c->cv.incl.p, c->cv.dep_tile.p, n_ev, c->cv.tile_last.p);
    k_cv_tails_top<<<1, CV_THREADS, 0, c->stream>>>(c->cv.tile_last.p, etiles, c->cv.tile_prev.p);
    k_cv_flag<<<etiles, CV_THREADS, 0, c->stream>>>(skey, c->cv.incl.p, c->cv.dep_tile.p, c->cv.tile_prev.p, n_ev, c->cv.mark.p, c->cv.cnt_tile.p, c->cv.part.p);
    k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->cv.cnt_tile.p, etiles, c->cv.stat.d + CV_ST_MARKS, c->cv.part.p, 1, 0, c->cv.stat.d + CV_ST_MAX_DEPTH);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->cv.ev[5], c->stream));
    HIPCHK(c->cv.stat.fetch(c->stream));
    HIPCHK(wait_stream(c));                                       // the second wait: how many breakpoints and entries
    const size_t n_bp = (size_t)(uint32_t)c->cv.stat.h[CV_ST_MARKS], n_ent = (size_t)(c->cv.stat.h[CV_ST_MARKS] >> 32);
    if ((uint32_t)c->cv.stat.h[CV_ST_DEPTH_END] != 0u || n_bp < 2 || n_ent < 1 || n_ent >= n_bp || n_bp > n_ev) {
        snprintf(c->err, 512, "%s: %u events leave the depth %u behind the last, %zu breakpoints and %zu entries", fn, n_ev, (uint32_t)c->cv.stat.h[CV_ST_DEPTH_END], n_bp, n_ent);
        return DG_ERR_INTERNAL;
    }
    const uint32_t ntiles = (uint32_t)((n_ent + CV_THREADS - 1) / CV_THREADS);
    BS_ENSURE(c->cv.bp_key, n_bp, "the breakpoints' keys"); BS_ENSURE(c->cv.bp_depth, n_bp, "the breakpoints' depths"); BS_ENSURE(c->cv.ent_bp, n_ent, "the entries' breakpoints");
    BS_ENSURE(c->cv.entries, n_ent, "the entries"); BS_ENSURE(c->cv.line_off, n_ent, "the lines' offsets"); BS_ENSURE(c->cv.line_tile, (size_t)ntiles + 1, "the per-workgroup line sums");
    BS_ENSURE(c->cv.part, 2 * (size_t)ntiles, "the per-workgroup values");
    {   // the chromosome names are read and the kernels that use them enqueued under the index's lock (as the SAM formatter does: dg_set_chr_names waits for the device before it frees them)
        std::unique_lock<std::mutex> lk;
        const uint32_t *name_off = nullptr; const char *names = nullptr;
        if (text) {
            lk = std::unique_lock<std::mutex>(sh->mu);
            name_off = sh->d_chr_name_off; names = sh->d_chr_names;
            BS_ENSURE(c->cv.text, (size_t)(n_ent * cv_line_bound(sh->chr_name_max)), "the text");
        }
        HIPCHK(hipEventRecord(c->cv.ev[6], c->stream));
        k_cv_compact<<<etiles, CV_THREADS, 0, c->stream>>>(skey, c->cv.incl.p, c->cv.dep_tile.p, c->cv.mark.p, c->cv.cnt_tile.p, n_ev, (uint32_t)n_bp, (uint32_t)n_ent, c->cv.bp_key.p, c->cv.bp_depth.p, c->cv.ent_bp.p);
        HIPCHK(hipEventRecord(c->cv.ev[7], c->stream));
        k_cv_entries<<<ntiles, CV_THREADS, 0, c->stream>>>(c->cv.bp_key.p, c->cv.bp_depth.p, c->cv.ent_bp.p, (uint32_t)n_bp, (uint32_t)n_ent, n_chr, name_off, c->cv.entries.p, c->cv.line_off.p, c->cv.line_tile.p, c->cv.part.p);
        k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->cv.line_tile.p, ntiles, c->cv.stat.d + CV_ST_BYTES, c->cv.part.p, 2, 2, c->cv.stat.d + CV_ST_COVERED);
        if (text)
            k_cv_write<<<ntiles, CV_THREADS, 0, c->stream>>>(c->cv.entries.p, (uint32_t)n_ent, n_chr, name_off, names, c->cv.line_off.p, c->cv.line_tile.p, c->cv.stat.d, (unsigned long long)c->cv.text.cap, c->cv.text.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->cv.ev[8], c->stream));
    }
    HIPCHK(c->cv.stat.fetch(c->stream));
    HIPCHK(wait_stream(c));                                       // the third wait: the text's size, the covered bases
    const size_t bytes = text ? (size_t)c->cv.stat.h[CV_ST_BYTES] : 0;
    if (bytes > c->cv.text.cap) { snprintf(c->err, 512, "%s: the text needs %zu bytes, the bound was %zu", fn, bytes, c->cv.text.cap); return DG_ERR_INTERNAL; }
    if (c->cv.stat.h[CV_ST_AREA] != aligned) { snprintf(c->err, 512, "%s: the entries hold %llu aligned bases, the blocks %llu", fn, c->cv.stat.h[CV_ST_AREA], aligned); return DG_ERR_INTERNAL; }
    c->cv.ms[1] = c->cv.ev.ms(2, 3); c->cv.ms[2] = c->cv.ev.ms(3, 4); c->cv.ms[3] = c->cv.ev.ms(4, 5) + c->cv.ev.ms(6, 7); c->cv.ms[4] = c->cv.ev.ms(7, 8);
    return done(n_ent, bytes, n_bp, c->cv.stat.h[CV_ST_COVERED], c->cv.stat.h[CV_ST_MAX_DEPTH]);
}

// ---- the accessors of the two table stages (the coverage track, the allele counts): S = CvState / PuState; the function is dg_bam_<stage>_<call>, `noun` what
// its texts call the result ----
template <class S, class E>
static int table_download(dg_ctx *c, S dg_ctx::*m, const char *stage, const char *noun, E *entries, size_t cap_entries, char *text, size_t cap_text)
{
    if (!c) return DG_ERR_ARG;
    S &st = c->*m;
    if (!st.valid || !c->bs.fin_valid) { snprintf(c->err, 512, "dg_bam_%s_download: no %s (dg_bam_%s_finish first, and no store call behind it)", stage, noun, stage); return DG_ERR_ARG; }
    if ((entries && cap_entries < st.n_entries) || (text && cap_text < st.bytes)) {
        snprintf(c->err, 512, "dg_bam_%s_download: output capacity too small: %zu entries and %zu bytes of text are needed", stage, st.n_entries, st.bytes);
        return DG_ERR_CAPACITY;
    }
    HIPCHK(hipSetDevice(c->device));
    if (entries && st.n_entries) HIPCHK(hipMemcpyAsync(entries, st.entries.p, st.n_entries * sizeof(E), hipMemcpyDeviceToHost, c->stream));
    if (text && st.bytes) HIPCHK(hipMemcpyAsync(text, st.text.p, st.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));
    return DG_OK;
}
template <class S>
static int table_device(dg_ctx *c, S dg_ctx::*m, const char *stage, const char *noun, void **entries, void **text)
{
    if (!c) return DG_ERR_ARG;
    S &st = c->*m;
    if (!st.valid || !c->bs.fin_valid) { snprintf(c->err, 512, "dg_bam_%s_device: no %s (dg_bam_%s_finish first, and no store call behind it)", stage, noun, stage); return DG_ERR_ARG; }
    if (entries) *entries = st.n_entries ? st.entries.p : nullptr;
    if (text) *text = st.bytes ? st.text.p : nullptr;
    return DG_OK;
}
template <class S>
static int table_device_ms(dg_ctx *c, S dg_ctx::*m, float ms[5], int *n_passes)
{
    if (!c || !ms) return DG_ERR_ARG;
    for (int k = 0; k < 5; k++) ms[k] = (c->*m).ms[k];
    if (n_passes) *n_passes = (c->*m).passes;
    return DG_OK;
}

extern "C" int dg_bam_coverage_download(dg_ctx *c, dg_cov_entry *entries, size_t cap_entries, char *text, size_t cap_text) { return table_download(c, &dg_ctx::cv, "coverage", "track", entries, cap_entries, text, cap_text); }
extern "C" int dg_bam_coverage_device(dg_ctx *c, void **entries, void **text) { return table_device(c, &dg_ctx::cv, "coverage", "track", entries, text); }
extern "C" int dg_bam_coverage_device_ms(dg_ctx *c, float ms[5], int *n_passes) { return table_device_ms(c, &dg_ctx::cv, ms, n_passes); }

// ------------------------------------------------------------------------------------------
// the allele counts of the sorted array (dg_pileup.h): the records' bases against the index's 2-bit text, in buffers of its own
// ------------------------------------------------------------------------------------------
extern "C" int dg_bam_pileup_granules(int out[3])
{
    if (!out) return DG_ERR_ARG;
    out[0] = PU_WG; out[1] = RS_TILE; out[2] = PU_STEP;
    return DG_OK;
}

extern "C" int dg_bam_pileup_finish(dg_ctx *c, uint32_t flags, uint32_t exclude_flags, uint32_t min_mapq, uint32_t min_alt, size_t *n_sites, size_t *n_bytes, uint64_t stats[10], float *device_ms)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_bam_pileup_finish";
    if (n_sites) *n_sites = 0;
    if (n_bytes) *n_bytes = 0;
    if (device_ms) *device_ms = 0.f;
    if (stats) for (int k = 0; k < 10; k++) stats[k] = 0;
    c->pu.valid = false; c->pu.n_entries = 0; c->pu.bytes = 0; c->pu.passes = 0;
    for (float &m : c->pu.ms) m = 0.f;
    BsView sv;
    { const int rc = bs_view(c, fn, sv); if (rc) return rc; }
    if (flags & ~DG_PU_ENTRIES_ONLY) { snprintf(c->err, 512, "%s: flags 0x%x hold a bit that is not DG_PU_ENTRIES_ONLY", fn, flags); return DG_ERR_ARG; }
    if (min_alt == 0u) { snprintf(c->err, 512, "%s: min_alt is 0: a site has at least one observation of its top allele", fn); return DG_ERR_ARG; }
    const bool text = !(flags & DG_PU_ENTRIES_ONLY);
    IndexShared *sh = c->shared_ix;
    if (text && (!sh || !sh->chr_names_set)) { snprintf(c->err, 512, "%s: the chromosome names are missing (dg_set_chr_names), and DG_PU_ENTRIES_ONLY is not set", fn); return DG_ERR_ARG; }
    HIPCHK(c->pu.ready());
    const size_t n = sv.n, n_raw = sv.n_raw;
    const int n_chr = sv.n_chr;
    if (n_chr < 1) { snprintf(c->err, 512, "%s: %d chromosomes", fn, n_chr); return DG_ERR_ARG; }
    if (!n) { c->pu.valid = true; return DG_OK; }
    const PuFilter f{exclude_flags, min_mapq};
    const DIndex ix = c->ix;
    const uint32_t tiles = (uint32_t)((n + PU_WG - 1) / PU_WG);
    BS_ENSURE(c->pu.ev_off, n, "the records' event offsets"); BS_ENSURE(c->pu.ev_tile, (size_t)tiles + 1, "the per-workgroup event counts");
    BS_ENSURE(c->pu.junk, (size_t)tiles + 1, "the per-workgroup scratch"); BS_ENSURE(c->pu.part, (size_t)CV_PLANES * tiles, "the per-workgroup values");
    BS_ENSURE(c->pu.part2, 2 * (size_t)tiles, "the per-workgroup key bounds");
    HIPCHK(hipMemsetAsync(c->pu.stat.d, 0, PU_ST_WORDS * 8, c->stream));
    HIPCHK(hipMemsetAsync(c->pu.junk.p, 0, ((size_t)tiles + 1) * 8, c->stream));
    HIPCHK(hipEventRecord(c->pu.ev[0], c->stream));
    k_pu_count<<<tiles, PU_WG, 0, c->stream>>>(sv.rec, sv.dst_off, sv.tile, (uint32_t)n, (unsigned long long)n_raw, ix, f, c->pu.ev_off.p, c->pu.ev_tile.p, c->pu.part.p, c->pu.part2.p);
    k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->pu.ev_tile.p, tiles, c->pu.stat.d + PU_ST_EVENTS, c->pu.part.p, 5, 4, c->pu.stat.d + PU_ST_RECS);
    k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->pu.junk.p, tiles, c->pu.stat.d + PU_ST_JUNK, c->pu.part2.p, 2, 0, c->pu.stat.d + PU_ST_NMIN);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->pu.ev[1], c->stream));
    HIPCHK(c->pu.stat.fetch(c->stream));
    HIPCHK(wait_stream(c));                                       // the first wait: how many events, the bounds of their keys, and what was out of range
    const unsigned long long *st = c->pu.stat.h;
    if (st[PU_ST_NBAD]) {
        snprintf(c->err, 512, "%s: record %llu of the sorted array has a block that ends behind position 2^32 - 1: an entry cannot hold it; no table was built", fn, ~st[PU_ST_NBAD]);
        return DG_ERR_RANGE;
    }
    const unsigned long long n_events = st[PU_ST_EVENTS];
    if (n_events >= 0xFFFFF000ull) { snprintf(c->err, 512, "%s: %llu events are more than the sorter takes (2^32 - 1, less a tile)", fn, n_events); return DG_ERR_CAPACITY; }
    // (fewer than 2^32 events: every counter below is below 2^32, and the packed sums did not run into each other)
    const unsigned long long n_counted = (uint32_t)st[PU_ST_RECS], n_left_out = st[PU_ST_RECS] >> 32, aligned = st[PU_ST_ALIGNED], n_blocks = (uint32_t)st[PU_ST_BLK_INS], n_ins = st[PU_ST_BLK_INS] >> 32,
                             n_mis = (uint32_t)st[PU_ST_MIS_DEL], n_del = st[PU_ST_MIS_DEL] >> 32;
    c->pu.ms[0] = c->pu.ev.ms(0, 1);
    auto done = [&](size_t n_before, size_t n_kept, size_t nb, unsigned long long deepest) {
        float total = 0.f;
        for (float m : c->pu.ms) total += m;
        c->pu.valid = true; c->pu.n_entries = n_kept; c->pu.bytes = nb;
        if (n_sites) *n_sites = n_kept;
        if (n_bytes) *n_bytes = nb;
        if (device_ms) *device_ms = total;
        if (stats) { stats[0] = n_counted; stats[1] = n_blocks; stats[2] = aligned; stats[3] = n_mis; stats[4] = n_del; stats[5] = n_ins; stats[6] = n_before; stats[7] = n_kept; stats[8] = n_left_out; stats[9] = deepest; }
        return DG_OK;
    };
    if (n_events != 2 * n_blocks + n_mis + n_del + n_ins) { snprintf(c->err, 512, "%s: %llu events, but %llu blocks, %llu mismatches, %llu deleted bases and %llu insertions", fn, n_events, n_blocks, n_mis, n_del, n_ins); return DG_ERR_INTERNAL; }
    if (n_events == 2 * n_blocks) return done(0, 0, 0, 0);        // (no allele event: no site; this covers no event at all)
    const uint32_t n_ev = (uint32_t)n_events, etiles = (n_ev + PU_WG - 1) / PU_WG;
    for (int k = 0; k < 2; k++) { BS_ENSURE(c->pu.sort.k[k], (size_t)n_ev, "the events' keys"); BS_ENSURE(c->pu.sort.v[k], (size_t)n_ev, "the events' values"); }
    BS_ENSURE_SORT(c->pu.sort, n_ev);
    BS_ENSURE(c->pu.incl_d, (size_t)n_ev, "the scanned depth plane"); BS_ENSURE(c->pu.incl_a, (size_t)n_ev, "the scanned allele plane");
    BS_ENSURE(c->pu.prev_tail, (size_t)n_ev, "the events' previous tails"); BS_ENSURE(c->pu.mark, (size_t)n_ev, "the events' marks");
    BS_ENSURE(c->pu.tile_d, (size_t)etiles + 1, "the per-workgroup depth sums"); BS_ENSURE(c->pu.tile_a, (size_t)etiles + 1, "the per-workgroup allele sums");
    BS_ENSURE(c->pu.tile_last, (size_t)etiles + 1, "the per-workgroup last tails"); BS_ENSURE(c->pu.tile_prev, (size_t)etiles + 1, "the per-workgroup previous tails");
    BS_ENSURE(c->pu.cnt_tile, (size_t)etiles + 1, "the per-workgroup key counts");
    const int bits = std::min(cv_key_bits(~st[PU_ST_NMIN], st[PU_ST_MAX]), pu_key_bits_max(n_chr));
    int which = 0;
    HIPCHK(hipEventRecord(c->pu.ev[2], c->stream));
    k_pu_emit<<<tiles, PU_WG, 0, c->stream>>>(sv.rec, sv.dst_off, sv.tile, (uint32_t)n, (unsigned long long)n_raw, ix, f, c->pu.ev_off.p, c->pu.ev_tile.p, n_events, c->pu.sort.k[0].p, c->pu.sort.v[0].p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->pu.ev[3], c->stream));
    {
        const int rc = c->pu.sort.sort(c, n_ev, bits, which);
        if (rc) return rc;
        c->pu.passes = (bits + 3) / 4;
    }
    HIPCHK(hipEventRecord(c->pu.ev[4], c->stream));
    const uint64_t *skey = c->pu.sort.k[which].p;
    k_pu_scan<<<etiles, PU_WG, 0, c->stream>>>(skey, c->pu.sort.v[which].p, n_ev, c->pu.incl_d.p, c->pu.incl_a.p, c->pu.tile_d.p, c->pu.tile_a.p);
    k_tiles_top<uint64_t><<<1, 256, 0, c->stream>>>(c->pu.tile_d.p, etiles, (uint64_t *)(c->pu.stat.d + PU_ST_DEPTH_END));
    k_tiles_top<uint64_t><<<1, 256, 0, c->stream>>>(c->pu.tile_a.p, etiles, (uint64_t *)(c->pu.stat.d + PU_ST_ALLELES));
    k_pu_tails<<<etiles, PU_WG, 0, c->stream>>>(skey, n_ev, c->pu.tile_last.p);
    k_cv_tails_top<<<1, CV_THREADS, 0, c->stream>>>(c->pu.tile_last.p, etiles, c->pu.tile_prev.p);
    k_pu_flag<<<etiles, PU_WG, 0, c->stream>>>(skey, c->pu.tile_prev.p, n_ev, c->pu.prev_tail.p, c->pu.mark.p, c->pu.cnt_tile.p);
    k_tiles_top<uint64_t><<<1, 256, 0, c->stream>>>(c->pu.cnt_tile.p, etiles, (uint64_t *)(c->pu.stat.d + PU_ST_MARKS));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->pu.ev[5], c->stream));
    HIPCHK(c->pu.stat.fetch(c->stream));
    HIPCHK(wait_stream(c));                                       // the second wait: how many distinct allele keys and sites
    const size_t n_keys = (size_t)(uint32_t)st[PU_ST_MARKS], n_before = (size_t)(st[PU_ST_MARKS] >> 32);
    const unsigned long long alleles = st[PU_ST_ALLELES];
    if (st[PU_ST_DEPTH_END] != 0ull || (unsigned long long)(uint32_t)alleles != n_mis + n_del + n_ins || n_before < 1 || n_before > n_keys || n_keys > n_mis + n_del + n_ins) {
        snprintf(c->err, 512, "%s: %u events leave the depth 0x%llx behind the last and %llu allele events of %llu, %zu distinct allele keys and %zu sites", fn, n_ev, st[PU_ST_DEPTH_END],
                 (unsigned long long)(uint32_t)alleles, n_mis + n_del + n_ins, n_keys, n_before);
        return DG_ERR_INTERNAL;
    }
    const uint32_t stiles = (uint32_t)((n_before + PU_WG - 1) / PU_WG);
    BS_ENSURE(c->pu.ak_key, n_keys, "the allele keys"); BS_ENSURE(c->pu.ak_n, n_keys, "the allele keys' counts"); BS_ENSURE(c->pu.ak_depth, n_keys, "the allele keys' depths");
    BS_ENSURE(c->pu.site_key, n_before, "the sites' first keys"); BS_ENSURE(c->pu.site_mark, n_before, "the sites' marks"); BS_ENSURE(c->pu.line_off, n_before, "the lines' offsets");
    BS_ENSURE(c->pu.kept_tile, (size_t)stiles + 1, "the per-workgroup site counts"); BS_ENSURE(c->pu.line_tile, (size_t)stiles + 1, "the per-workgroup line sums");
    BS_ENSURE(c->pu.part, (size_t)stiles, "the per-workgroup values");
    // the chromosome names are read and the kernels that use them enqueued under the index's lock, as the coverage track does; the lock is held across the third wait,
    // whose sizes the writing kernel needs
    std::unique_lock<std::mutex> lk;
    const uint32_t *name_off = nullptr; const char *names = nullptr;
    if (text) { lk = std::unique_lock<std::mutex>(sh->mu); name_off = sh->d_chr_name_off; names = sh->d_chr_names; }
    HIPCHK(hipEventRecord(c->pu.ev[6], c->stream));
    k_pu_compact<<<etiles, PU_WG, 0, c->stream>>>(skey, c->pu.incl_d.p, c->pu.incl_a.p, c->pu.tile_d.p, c->pu.tile_a.p, c->pu.prev_tail.p, c->pu.mark.p, c->pu.cnt_tile.p, n_ev, (uint32_t)n_keys,
                                                   (uint32_t)n_before, c->pu.ak_key.p, c->pu.ak_n.p, c->pu.ak_depth.p, c->pu.site_key.p);
    HIPCHK(hipEventRecord(c->pu.ev[7], c->stream));
    k_pu_sites<<<stiles, PU_WG, 0, c->stream>>>(c->pu.ak_key.p, c->pu.ak_n.p, c->pu.ak_depth.p, c->pu.site_key.p, (uint32_t)n_keys, (uint32_t)n_before, ix, min_alt, name_off, c->pu.site_mark.p,
                                                 c->pu.line_off.p, c->pu.kept_tile.p, c->pu.line_tile.p, c->pu.part.p);
    k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->pu.kept_tile.p, stiles, c->pu.stat.d + PU_ST_KEPT, c->pu.part.p, 1, 0, c->pu.stat.d + PU_ST_MAX_DEPTH);
    k_tiles_top<uint64_t><<<1, 256, 0, c->stream>>>(c->pu.line_tile.p, stiles, (uint64_t *)(c->pu.stat.d + PU_ST_BYTES));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->pu.ev[8], c->stream));
    HIPCHK(c->pu.stat.fetch(c->stream));
    HIPCHK(wait_stream(c));                                       // the third wait: the kept sites and the text's size
    const size_t n_kept = (size_t)st[PU_ST_KEPT], bytes = text ? (size_t)st[PU_ST_BYTES] : 0;
    if (n_kept > n_before) { snprintf(c->err, 512, "%s: %zu sites kept of %zu", fn, n_kept, n_before); return DG_ERR_INTERNAL; }
    HIPCHK(hipEventRecord(c->pu.ev[9], c->stream));
    if (n_kept) {
        BS_ENSURE(c->pu.entries, n_kept, "the entries");
        if (bytes) BS_ENSURE(c->pu.text, bytes, "the text");
        k_pu_write<<<stiles, PU_WG, 0, c->stream>>>(c->pu.ak_key.p, c->pu.ak_n.p, c->pu.ak_depth.p, c->pu.site_key.p, (uint32_t)n_keys, (uint32_t)n_before, ix, min_alt, name_off, bytes ? names : nullptr,
                                                     c->pu.site_mark.p, c->pu.line_off.p, c->pu.kept_tile.p, c->pu.line_tile.p, (unsigned long long)n_kept, (unsigned long long)bytes, c->pu.entries.p,
                                                     c->pu.text.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(c->pu.ev[10], c->stream));
    HIPCHK(wait_stream(c));
    c->pu.ms[1] = c->pu.ev.ms(2, 3); c->pu.ms[2] = c->pu.ev.ms(3, 4); c->pu.ms[3] = c->pu.ev.ms(4, 5) + c->pu.ev.ms(6, 7); c->pu.ms[4] = c->pu.ev.ms(7, 8) + c->pu.ev.ms(9, 10);
    return done(n_before, n_kept, bytes, st[PU_ST_MAX_DEPTH]);
}

extern "C" int dg_bam_pileup_download(dg_ctx *c, dg_site_entry *entries, size_t cap_entries, char *text, size_t cap_text) { return table_download(c, &dg_ctx::pu, "pileup", "table", entries, cap_entries, text, cap_text); }
extern "C" int dg_bam_pileup_device(dg_ctx *c, void **entries, void **text) { return table_device(c, &dg_ctx::pu, "pileup", "table", entries, text); }
extern "C" int dg_bam_pileup_device_ms(dg_ctx *c, float ms[5], int *n_passes) { return table_device_ms(c, &dg_ctx::pu, ms, n_passes); }

// ------------------------------------------------------------------------------------------
// the QC tables of the sorted array (dg_qc.h): one flat array of counters, both kernels add into it; read-only on the sorted array
// ------------------------------------------------------------------------------------------
extern "C" int dg_bam_qc_granules(int out[5])
{
    if (!out) return DG_ERR_ARG;
    out[0] = QC_WG; out[1] = QC_LANE_BASES; out[2] = QC_STEP; out[3] = QC_FLUSH_TRIPS; out[4] = (int)QC_BIG;
    return DG_OK;
}

extern "C" int dg_bam_qc_offsets(int n_chr, size_t out[9])
{
    if (!out || n_chr < 1) return DG_ERR_ARG;
    out[0] = qc_off_fs(); out[1] = qc_off_ch(); out[2] = qc_off_mq(n_chr); out[3] = qc_off_is(n_chr); out[4] = qc_off_rl(n_chr); out[5] = qc_off_pc(n_chr); out[6] = qc_off_id(n_chr);
    out[7] = qc_off_sn(n_chr); out[8] = qc_words(n_chr);
    return DG_OK;
}

extern "C" int dg_bam_qc_format(const uint64_t *words, size_t n_words, int n_chr, const char *const *names, const int64_t *lengths, char *out, size_t cap, size_t *n_bytes)
{
    if (n_bytes) *n_bytes = 0;
    if (!words || !names || !lengths || n_chr < 1 || n_words != qc_words(n_chr) || (!out && cap)) return DG_ERR_ARG;
    std::string text;
    qc_format(words, n_chr, names, lengths, text);
    if (n_bytes) *n_bytes = text.size();
    if (cap < text.size()) return DG_ERR_CAPACITY;
    if (!text.empty()) memcpy(out, text.data(), text.size());
    return DG_OK;
}

extern "C" int dg_bam_qc_finish(dg_ctx *c, uint32_t flags, uint32_t exclude_flags, uint32_t min_mapq, size_t *n_words, float *device_ms)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_bam_qc_finish";
    if (n_words) *n_words = 0;
    if (device_ms) *device_ms = 0.f;
    c->qc.valid = false; c->qc.n_words = 0; c->qc.ms[0] = c->qc.ms[1] = 0.f;
    BsView sv;
    { const int rc = bs_view(c, fn, sv); if (rc) return rc; }
    if (flags) { snprintf(c->err, 512, "%s: flags 0x%x hold a bit that is not defined", fn, flags); return DG_ERR_ARG; }
    HIPCHK(c->qc.ready());
    const size_t n = sv.n, n_raw = sv.n_raw;
    const int n_chr = sv.n_chr;
    if (n_chr < 1) { snprintf(c->err, 512, "%s: %d chromosomes", fn, n_chr); return DG_ERR_ARG; }
    const size_t nw = qc_words(n_chr);
    BS_ENSURE(c->qc.words, nw, "the tables");
    HIPCHK(hipMemsetAsync(c->qc.words.p, 0, nw * 8, c->stream));
    if (n) {
        const PuFilter f{exclude_flags, min_mapq};
        const DIndex ix = c->ix;
        const uint32_t cap = (uint32_t)c->qc.max_groups;
        const uint32_t g_flag = (uint32_t)std::min<size_t>(cap, (n + QC_WG - 1) / QC_WG), g_cycle = (uint32_t)std::min<size_t>(cap, (n + QC_WG / QC_GROUP - 1) / (QC_WG / QC_GROUP));
        HIPCHK(hipEventRecord(c->qc.ev[0], c->stream));
        k_qc_flag<<<g_flag, QC_WG, 0, c->stream>>>(sv.rec, sv.dst_off, sv.tile, (uint32_t)n, (unsigned long long)n_raw, n_chr, c->qc.words.p);
        HIPCHK(hipEventRecord(c->qc.ev[1], c->stream));
        k_qc_cycle<<<g_cycle, QC_WG, 0, c->stream>>>(sv.rec, sv.dst_off, sv.tile, (uint32_t)n, (unsigned long long)n_raw, ix, f, c->qc.words.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->qc.ev[2], c->stream));
    }
    HIPCHK(wait_stream(c));
    if (n) { c->qc.ms[0] = c->qc.ev.ms(0, 1); c->qc.ms[1] = c->qc.ev.ms(1, 2); }
    c->qc.valid = true; c->qc.n_words = nw;
    if (n_words) *n_words = nw;
    if (device_ms) *device_ms = c->qc.ms[0] + c->qc.ms[1];
    return DG_OK;
}

extern "C" int dg_bam_qc_download(dg_ctx *c, uint64_t *words, size_t cap_words)
{
    if (!c) return DG_ERR_ARG;
    if (!c->qc.valid || !c->bs.fin_valid) { snprintf(c->err, 512, "dg_bam_qc_download: no tables (dg_bam_qc_finish first, and no store call behind it)"); return DG_ERR_ARG; }
    if (!words || cap_words < c->qc.n_words) { snprintf(c->err, 512, "dg_bam_qc_download: output capacity too small: %zu words are needed", c->qc.n_words); return DG_ERR_CAPACITY; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(words, c->qc.words.p, c->qc.n_words * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));
    return DG_OK;
}

extern "C" int dg_bam_qc_device(dg_ctx *c, void **words)
{
    if (!c) return DG_ERR_ARG;
    if (!c->qc.valid || !c->bs.fin_valid) { snprintf(c->err, 512, "dg_bam_qc_device: no tables (dg_bam_qc_finish first, and no store call behind it)"); return DG_ERR_ARG; }
    if (words) *words = c->qc.words.p;
    return DG_OK;
}

extern "C" int dg_bam_qc_device_ms(dg_ctx *c, float ms[2])
{
    if (!c || !ms) return DG_ERR_ARG;
    ms[0] = c->qc.ms[0]; ms[1] = c->qc.ms[1];
    return DG_OK;
}

// ------------------------------------------------------------------------------------------
// the RNA-seq metrics of the sorted array (dg_rnametrics.h): the annotation's tables live with the index, the words and the event path's buffers with the
// context; read-only on the sorted array
// ------------------------------------------------------------------------------------------
extern "C" int dg_bam_rna_granules(int out[2])
{
    if (!out) return DG_ERR_ARG;
    out[0] = RM_THREADS; out[1] = RM_TX_PER_WG;
    return DG_OK;
}

extern "C" int dg_bam_rna_offsets(size_t out[6])
{
    if (!out) return DG_ERR_ARG;
    out[0] = rm_off_ba(); out[1] = rm_off_rc(); out[2] = rm_off_st(); out[3] = rm_off_bc(); out[4] = rm_off_sn(); out[5] = rm_words();
    return DG_OK;
}

extern "C" int dg_bam_rna_format(const uint64_t *words, size_t n_words, char *out, size_t cap, size_t *n_bytes)
{
    if (n_bytes) *n_bytes = 0;
    if (!words || n_words != rm_words() || (!out && cap)) return DG_ERR_ARG;
    std::string text;
    rm_format(words, text);
    if (n_bytes) *n_bytes = text.size();
    if (cap < text.size()) return DG_ERR_CAPACITY;
    if (!text.empty()) memcpy(out, text.data(), text.size());
    return DG_OK;
}

extern "C" int dg_rna_set_annotation(dg_ctx *c, const dg_rna_annot *a, size_t *n_segments, size_t *n_eligible)
{
    if (!c) return DG_ERR_ARG;
    if (n_segments) *n_segments = 0;
    if (n_eligible) *n_eligible = 0;
    IndexShared *sh = c->shared_ix;
    if (!sh || !a) { snprintf(c->err, 512, "dg_rna_set_annotation: no annotation (or a context without an index)"); return DG_ERR_ARG; }
    RmFlat fl;
    char why[400];
    if (!rm_flatten(c->ix.n_chr, a, fl, why, sizeof why)) { snprintf(c->err, 512, "dg_rna_set_annotation: %s", why); return DG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(sh->mu);
    void *d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const void *src[5] = {fl.chr_first.data(), fl.seg_start.data(), fl.seg_cs.data(), fl.tx.data(), fl.ex.data()};
    const size_t bytes[5] = {fl.chr_first.size() * 4, fl.seg_start.size() * 4, fl.seg_cs.size() * 4, fl.tx.size() * sizeof(RmTx), fl.ex.size() * sizeof(RmExon)};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 5 && e == hipSuccess; k++) {
        e = hipMalloc(&d[k], bytes[k] + 64);
        if (e == hipSuccess && bytes[k]) e = hipMemcpy(d[k], src[k], bytes[k], hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) { for (void *p : d) if (p) (void)hipFree(p); return fail(c, DG_ERR_HIP, "the transcript annotation's tables", e); }
    // dg_bam_rna_finish reads the pointers and enqueues the kernels that use them under sh->mu: under the lock every kernel that may read the old tables is
    // already in a stream, so the device is waited for, then they are freed (as dg_gene_set_annotation does)
    if (sh->rm_gen) { (void)hipDeviceSynchronize(); for (void *p : {(void *)sh->d_rm_chr_first, (void *)sh->d_rm_seg_start, (void *)sh->d_rm_seg_cs, (void *)sh->d_rm_tx, (void *)sh->d_rm_ex}) (void)hipFree(p); }
    sh->d_rm_chr_first = (uint32_t *)d[0]; sh->d_rm_seg_start = (uint32_t *)d[1]; sh->d_rm_seg_cs = (uint32_t *)d[2]; sh->d_rm_tx = (RmTx *)d[3]; sh->d_rm_ex = (RmExon *)d[4];
    sh->rm_n_seg = fl.seg_start.size(); sh->rm_n_tx = a->n_tx; sh->rm_n_elig = fl.tx.size(); sh->rm_gen++;
    if (n_segments) *n_segments = fl.seg_start.size();
    if (n_eligible) *n_eligible = fl.tx.size();
    return DG_OK;
}

extern "C" int dg_bam_rna_finish(dg_ctx *c, uint32_t flags, uint32_t exclude_flags, uint32_t min_mapq, uint64_t min_cov, size_t *n_words, float *device_ms)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_bam_rna_finish";
    if (n_words) *n_words = 0;
    if (device_ms) *device_ms = 0.f;
    c->rm.valid = false; c->rm.n_words = 0;
    for (float &m : c->rm.ms) m = 0.f;
    BsView sv;
    { const int rc = bs_view(c, fn, sv); if (rc) return rc; }
    if (flags) { snprintf(c->err, 512, "%s: flags 0x%x hold a bit that is not defined", fn, flags); return DG_ERR_ARG; }
    IndexShared *sh = c->shared_ix;
    uint64_t gen = 0;
    if (sh) { std::lock_guard<std::mutex> lk(sh->mu); gen = sh->rm_gen; }
    if (!gen) { snprintf(c->err, 512, "%s: no transcript annotation (dg_rna_set_annotation first)", fn); return DG_ERR_ARG; }
    HIPCHK(c->rm.ready());
    const size_t n = sv.n, n_raw = sv.n_raw;
    const int n_chr = sv.n_chr;
    if (n_chr < 1) { snprintf(c->err, 512, "%s: %d chromosomes", fn, n_chr); return DG_ERR_ARG; }
    const size_t nw = rm_words();
    const CvFilter f{0u, exclude_flags, min_mapq};
    const uint32_t tiles = (uint32_t)((n + CV_THREADS - 1) / CV_THREADS), cap = (uint32_t)c->rm.max_groups, g_class = std::min(cap, tiles);
    BS_ENSURE(c->rm.words, nw, "the words");
    BS_ENSURE(c->rm.line, (size_t)RM_PLANES * g_class + 1, "the per-workgroup lines");
    BS_ENSURE(c->rm.blk_off, n + 1, "the records' block offsets"); BS_ENSURE(c->rm.blk_tile, (size_t)tiles + 1, "the per-workgroup block counts");
    BS_ENSURE(c->rm.part, (size_t)CV_PLANES * tiles + 1, "the per-workgroup values");
    size_t n_elig = 0;
    HIPCHK(hipMemsetAsync(c->rm.words.p, 0, nw * 8, c->stream));
    HIPCHK(hipMemsetAsync(c->rm.stat.d, 0, CV_ST_WORDS * 8, c->stream));
    {   // the tables are read and the kernels that use them enqueued under the index's lock (dg_rna_set_annotation waits for the device before it frees them)
        std::lock_guard<std::mutex> lk(sh->mu);
        if (sh->rm_gen != gen) { snprintf(c->err, 512, "%s: the annotation was replaced while the call was being prepared", fn); return DG_ERR_ARG; }
        const RmTable t{sh->d_rm_chr_first, sh->d_rm_seg_start, sh->d_rm_seg_cs, n_chr};
        n_elig = sh->rm_n_elig;
        HIPCHK(hipEventRecord(c->rm.ev[0], c->stream));
        if (n) k_rm_class<<<g_class, RM_THREADS, 0, c->stream>>>(sv.rec, sv.dst_off, sv.tile, (uint32_t)n, (unsigned long long)n_raw, t, f, c->rm.line.p);
        k_rm_top<<<1, RM_THREADS, 0, c->stream>>>(c->rm.line.p, n ? g_class : 0u, (unsigned long long)n, (unsigned long long)sh->rm_n_tx, (unsigned long long)n_elig, (unsigned long long)sh->rm_n_seg, c->rm.words.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->rm.ev[1], c->stream));
    }
    if (n) {
        k_cv_count<<<tiles, CV_THREADS, 0, c->stream>>>(sv.rec, sv.dst_off, sv.tile, (uint32_t)n, (unsigned long long)n_raw, n_chr, f, c->rm.blk_off.p, c->rm.blk_tile.p, c->rm.part.p);
        k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->rm.blk_tile.p, tiles, c->rm.stat.d + CV_ST_BLOCKS, c->rm.part.p, 5, 2, c->rm.stat.d + CV_ST_COUNTED);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(c->rm.ev[2], c->stream));
    HIPCHK(c->rm.stat.fetch(c->stream));
    HIPCHK(wait_stream(c));                                       // the first wait: how many events, which digits their keys differ in, and what was out of range
    if (c->rm.stat.h[CV_ST_NBAD]) {
        snprintf(c->err, 512, "%s: record %llu of the sorted array has a block that ends behind position 2^32 - 1; no words were built", fn, ~c->rm.stat.h[CV_ST_NBAD]);
        return DG_ERR_RANGE;
    }
    const unsigned long long n_blocks = c->rm.stat.h[CV_ST_BLOCKS];
    if (2 * n_blocks >= 0xFFFFF000ull) { snprintf(c->err, 512, "%s: %llu events (two per block) are more than the sorter takes (2^32 - 1, less a tile)", fn, 2 * n_blocks); return DG_ERR_CAPACITY; }
    c->rm.ms[0] = c->rm.ev.ms(0, 1); c->rm.ms[1] = c->rm.ev.ms(1, 2);
    if (n_blocks && n_elig) {
        const uint32_t n_ev = (uint32_t)(2 * n_blocks), etiles = (n_ev + CV_THREADS - 1) / CV_THREADS;
        const uint32_t g_body = (uint32_t)std::min<size_t>(cap, (n_elig + RM_TX_PER_WG - 1) / RM_TX_PER_WG);
        for (int k = 0; k < 2; k++) { BS_ENSURE(c->rm.sort.k[k], (size_t)n_ev, "the events' keys"); BS_ENSURE(c->rm.sort.v[k], (size_t)n_ev, "the events' deltas"); }
        BS_ENSURE_SORT(c->rm.sort, n_ev);
        BS_ENSURE(c->rm.incl, (size_t)n_ev, "the scanned deltas"); BS_ENSURE(c->rm.dep_tile, (size_t)etiles + 1, "the per-workgroup depth sums");
        BS_ENSURE(c->rm.body, (size_t)RM_BODY_LINE * g_body, "the body pass's per-workgroup lines");
        const int bits = std::min(cv_key_bits(~c->rm.stat.h[CV_ST_NMIN], c->rm.stat.h[CV_ST_MAX]), cv_key_bits_max(n_chr));
        int which = 0;
        HIPCHK(hipEventRecord(c->rm.ev[3], c->stream));
        k_cv_emit<<<tiles, CV_THREADS, 0, c->stream>>>(sv.rec, sv.dst_off, sv.tile, (uint32_t)n, (unsigned long long)n_raw, n_chr, f, c->rm.blk_off.p, c->rm.blk_tile.p, n_blocks, c->rm.sort.k[0].p, c->rm.sort.v[0].p);
        HIPCHK(hipGetLastError());
        { const int rc = c->rm.sort.sort(c, n_ev, bits, which); if (rc) return rc; }
        k_cv_depth<<<etiles, CV_THREADS, 0, c->stream>>>(c->rm.sort.v[which].p, n_ev, c->rm.incl.p, c->rm.dep_tile.p);
        k_tiles_top<uint32_t><<<1, 256, 0, c->stream>>>(c->rm.dep_tile.p, etiles, (uint32_t *)(c->rm.stat.d + CV_ST_DEPTH_END));
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->rm.ev[4], c->stream));
        {
            std::lock_guard<std::mutex> lk(sh->mu);
            if (sh->rm_gen != gen) { snprintf(c->err, 512, "%s: the annotation was replaced while the call was running", fn); return DG_ERR_ARG; }
            k_rm_body<<<g_body, RM_THREADS, 0, c->stream>>>(sh->d_rm_tx, sh->d_rm_ex, (uint32_t)n_elig, c->rm.sort.k[which].p, c->rm.incl.p, c->rm.dep_tile.p, n_ev, (unsigned long long)min_cov, c->rm.body.p);
            k_rm_body_top<<<RM_BODY_LINE / RM_TX_PER_WG, RM_THREADS, 0, c->stream>>>(c->rm.body.p, g_body, c->rm.words.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(c->rm.ev[5], c->stream));
        }
        HIPCHK(c->rm.stat.fetch(c->stream));
        HIPCHK(wait_stream(c));                                   // the second wait
        if ((uint32_t)c->rm.stat.h[CV_ST_DEPTH_END] != 0u) { snprintf(c->err, 512, "%s: %u events leave the depth %u behind the last", fn, n_ev, (uint32_t)c->rm.stat.h[CV_ST_DEPTH_END]); return DG_ERR_INTERNAL; }
        c->rm.ms[1] += c->rm.ev.ms(3, 4); c->rm.ms[2] = c->rm.ev.ms(4, 5);
    }
    c->rm.valid = true; c->rm.n_words = nw;
    if (n_words) *n_words = nw;
    if (device_ms) *device_ms = c->rm.ms[0] + c->rm.ms[1] + c->rm.ms[2];
    return DG_OK;
}

extern "C" int dg_bam_rna_download(dg_ctx *c, uint64_t *words, size_t cap_words)
{
    if (!c) return DG_ERR_ARG;
    if (!c->rm.valid || !c->bs.fin_valid) { snprintf(c->err, 512, "dg_bam_rna_download: no words (dg_bam_rna_finish first, and no store call behind it)"); return DG_ERR_ARG; }
    if (!words || cap_words < c->rm.n_words) { snprintf(c->err, 512, "dg_bam_rna_download: output capacity too small: %zu words are needed", c->rm.n_words); return DG_ERR_CAPACITY; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(words, c->rm.words.p, c->rm.n_words * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(wait_stream(c));
    return DG_OK;
}

extern "C" int dg_bam_rna_device(dg_ctx *c, void **words)
{
    if (!c) return DG_ERR_ARG;
    if (!c->rm.valid || !c->bs.fin_valid) { snprintf(c->err, 512, "dg_bam_rna_device: no words (dg_bam_rna_finish first, and no store call behind it)"); return DG_ERR_ARG; }
    if (words) *words = c->rm.words.p;
    return DG_OK;
}

extern "C" int dg_bam_rna_device_ms(dg_ctx *c, float ms[3])
{
    if (!c || !ms) return DG_ERR_ARG;
    for (int k = 0; k < 3; k++) ms[k] = c->rm.ms[k];
    return DG_OK;
}

// ------------------------------------------------------------------------------------------
// duplicate marking of the sorted array (dg_markdup.h): flag 0x400 written in place, in HBM, before dg_bam_sort_compress
// ------------------------------------------------------------------------------------------
extern "C" int dg_bam_markdup_granules(int out[3])
{
    if (!out) return DG_ERR_ARG;
    out[0] = MD_THREADS; out[1] = RS_TILE; out[2] = MD_CROWD;
    return DG_OK;
}

extern "C" int dg_bam_markdup_finish(dg_ctx *c, uint32_t flags, uint64_t stats[8], float *device_ms)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_bam_markdup_finish";
    if (device_ms) *device_ms = 0.f;
    if (stats) for (int k = 0; k < 8; k++) stats[k] = 0;
    c->md.passes = 0;
    for (float &m : c->md.ms) m = 0.f;
    BsView sv;
    { const int rc = bs_view(c, fn, sv); if (rc) return rc; }
    if (flags & ~DG_MD_COUNT_ONLY) { snprintf(c->err, 512, "%s: flags 0x%x hold a bit that is not DG_MD_COUNT_ONLY", fn, flags); return DG_ERR_ARG; }
    const int write = (flags & DG_MD_COUNT_ONLY) ? 0 : 1;
    HIPCHK(c->md.ready());
    const size_t n = sv.n, n_raw = sv.n_raw;
    const int n_chr = sv.n_chr, hash_bits = c->md.hash_bits;
    if (n_chr < 1) { snprintf(c->err, 512, "%s: %d chromosomes", fn, n_chr); return DG_ERR_ARG; }
    if (!n) return DG_OK;
    const uint32_t tiles = (uint32_t)((n + MD_THREADS - 1) / MD_THREADS);
    BS_ENSURE(c->md.E, n, "the records' end keys"); BS_ENSURE(c->md.h, n, "the names' hashes"); BS_ENSURE(c->md.score, n, "the records' scores"); BS_ENSURE(c->md.mate, n, "the records' partners");
    BS_ENSURE(c->md.cand_off, n, "the candidates' offsets"); BS_ENSURE(c->md.cnt_off, n, "the pairs' and ends' offsets");
    BS_ENSURE(c->md.tile, (size_t)tiles + 1, "the per-workgroup sums"); BS_ENSURE(c->md.junk, (size_t)tiles + 1, "the per-workgroup sums"); BS_ENSURE(c->md.part, 2 * (size_t)tiles, "the per-workgroup values");
    BS_ENSURE(c->md.tile_last, (size_t)tiles + 1, "the per-workgroup last heads"); BS_ENSURE(c->md.tile_prev, (size_t)tiles + 2, "the per-workgroup previous heads");
    HIPCHK(hipMemsetAsync(c->md.stat.d, 0, MD_ST_WORDS * 8, c->stream));
    HIPCHK(hipMemsetAsync(c->md.junk.p, 0, ((size_t)tiles + 1) * 8, c->stream));
    HIPCHK(hipEventRecord(c->md.ev[0], c->stream));
    k_md_rec<<<tiles, MD_THREADS, 0, c->stream>>>(sv.rec, sv.dst_off, sv.tile, (uint32_t)n, (unsigned long long)n_raw, n_chr, hash_bits, c->md.E.p, c->md.h.p, c->md.score.p, c->md.mate.p,
                                                  c->md.cand_off.p, c->md.tile.p, c->md.part.p);
    k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->md.tile.p, tiles, c->md.stat.d + MD_ST_CAND, c->md.part.p, 2, 1, c->md.stat.d + MD_ST_EXAMINED);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->md.ev[1], c->stream));
    HIPCHK(c->md.stat.fetch(c->stream));
    HIPCHK(wait_stream(c));                                       // the first wait: how many candidates, and what was out of range
    if (c->md.stat.h[MD_ST_NBAD]) {
        snprintf(c->err, 512, "%s: record %llu of the sorted array has an unclipped 5' end outside [-2^31, 3 * 2^31): an end key cannot hold it; nothing was written", fn, ~c->md.stat.h[MD_ST_NBAD]);
        return DG_ERR_RANGE;
    }
    const size_t n_cand = (size_t)c->md.stat.h[MD_ST_CAND], n_examined = (size_t)c->md.stat.h[MD_ST_EXAMINED];
    if (n_cand > n || n_examined > n) { snprintf(c->err, 512, "%s: %zu candidates and %zu examined records of %zu", fn, n_cand, n_examined, n); return DG_ERR_INTERNAL; }
    const uint32_t ctiles = (uint32_t)((n_cand + MD_THREADS - 1) / MD_THREADS);
    SortBufs &ps = c->md.sort, &es = c->md.esort;          // candidates, then pairs / ends
    int which = 0;
    if (n_cand) {
        for (int k = 0; k < 2; k++) { BS_ENSURE(ps.k[k], n_cand, "the sorter's keys"); BS_ENSURE(ps.v[k], n_cand, "the sorter's values"); }
        BS_ENSURE_SORT(ps, (uint32_t)n_cand);
    }
    HIPCHK(hipEventRecord(c->md.ev[2], c->stream));
    if (n_cand) {
        k_md_compact<<<tiles, MD_THREADS, 0, c->stream>>>(c->md.cand_off.p, c->md.tile.p, c->md.h.p, (uint32_t)n, (uint32_t)n_cand, ps.k[0].p, ps.v[0].p);
        { const int rc = ps.sort(c, (uint32_t)n_cand, hash_bits, which); if (rc) return rc; }
        c->md.passes += (hash_bits + 3) / 4;
        k_md_mate<<<ctiles, MD_THREADS, 0, c->stream>>>(ps.k[which].p, ps.v[which].p, (uint32_t)n_cand, (uint32_t)n, sv.rec, sv.dst_off, sv.tile, c->md.mate.p, c->md.part.p);
        k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->md.junk.p, ctiles, c->md.stat.d + MD_ST_JUNK, c->md.part.p, 1, 1, c->md.stat.d + MD_ST_CROWDED);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(c->md.ev[3], c->stream));
    k_md_count<<<tiles, MD_THREADS, 0, c->stream>>>(c->md.mate.p, (uint32_t)n, c->md.cnt_off.p, c->md.tile.p);
    k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->md.tile.p, tiles, c->md.stat.d + MD_ST_COUNTS, nullptr, 0, 0, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->md.ev[4], c->stream));
    HIPCHK(c->md.stat.fetch(c->stream));
    HIPCHK(wait_stream(c));                                       // the second wait: how many pairs and ends
    const size_t n_pairs = (size_t)(c->md.stat.h[MD_ST_COUNTS] >> 32), n_ends = (size_t)(uint32_t)c->md.stat.h[MD_ST_COUNTS], n_crowded = (size_t)c->md.stat.h[MD_ST_CROWDED];
    if (2 * n_pairs > n_cand || n_ends != n_examined) { snprintf(c->err, 512, "%s: %zu pairs of %zu candidates, %zu ends of %zu examined records", fn, n_pairs, n_cand, n_ends, n_examined); return DG_ERR_INTERNAL; }
    const uint32_t ptiles = (uint32_t)((n_pairs + MD_THREADS - 1) / MD_THREADS), etiles = (uint32_t)((n_ends + MD_THREADS - 1) / MD_THREADS);
    if (n_ends) {
        for (int k = 0; k < 2; k++) { BS_ENSURE(es.k[k], n_ends, "the ends' keys"); BS_ENSURE(es.v[k], n_ends, "the ends' values"); }
        BS_ENSURE_SORT(es, (uint32_t)n_ends);
    }
    const int e_bits = md_e_bits(n_chr);
    int pw = 0, ew = 0;
    HIPCHK(hipEventRecord(c->md.ev[5], c->stream));
    if (n_ends) k_md_emit<<<tiles, MD_THREADS, 0, c->stream>>>(c->md.mate.p, c->md.score.p, c->md.cnt_off.p, c->md.tile.p, (uint32_t)n, (uint32_t)n_pairs, (uint32_t)n_ends, ps.k[0].p, ps.v[0].p, es.k[0].p, es.v[0].p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->md.ev[6], c->stream));
    if (n_pairs) {
        { const int rc = ps.sort(c, (uint32_t)n_pairs, MD_SCORE_BITS, pw); if (rc) return rc; }
        k_md_rekey<<<ptiles, MD_THREADS, 0, c->stream>>>(ps.k[pw].p, ps.v[pw].p, (uint32_t)n_pairs, 0, c->md.E.p, c->md.mate.p, (uint32_t)n);
        { const int rc = ps.sort(c, (uint32_t)n_pairs, e_bits, pw); if (rc) return rc; }
        k_md_rekey<<<ptiles, MD_THREADS, 0, c->stream>>>(ps.k[pw].p, ps.v[pw].p, (uint32_t)n_pairs, 1, c->md.E.p, c->md.mate.p, (uint32_t)n);
        { const int rc = ps.sort(c, (uint32_t)n_pairs, e_bits, pw); if (rc) return rc; }
        c->md.passes += (MD_SCORE_BITS + 3) / 4 + 2 * ((e_bits + 3) / 4);
    }
    HIPCHK(hipEventRecord(c->md.ev[7], c->stream));
    if (n_ends) {
        { const int rc = es.sort(c, (uint32_t)n_ends, MD_SCORE_BITS, ew); if (rc) return rc; }
        k_md_rekey<<<etiles, MD_THREADS, 0, c->stream>>>(es.k[ew].p, es.v[ew].p, (uint32_t)n_ends, 2, c->md.E.p, c->md.mate.p, (uint32_t)n);
        { const int rc = es.sort(c, (uint32_t)n_ends, e_bits, ew); if (rc) return rc; }
        c->md.passes += (MD_SCORE_BITS + 3) / 4 + (e_bits + 3) / 4;
    }
    HIPCHK(hipEventRecord(c->md.ev[8], c->stream));
    if (n_pairs) {
        k_md_heads<<<ptiles, MD_THREADS, 0, c->stream>>>(ps.k[pw].p, ps.v[pw].p, (uint32_t)n_pairs, c->md.E.p, c->md.mate.p, c->md.tile_last.p);
        k_cv_tails_top<<<1, CV_THREADS, 0, c->stream>>>(c->md.tile_last.p, ptiles, c->md.tile_prev.p);
        k_md_flag_pairs<<<ptiles, MD_THREADS, 0, c->stream>>>(ps.k[pw].p, ps.v[pw].p, (uint32_t)n_pairs, c->md.E.p, c->md.mate.p, c->md.tile_prev.p, sv.rec, sv.dst_off, sv.tile, (uint32_t)n,
                                                               (unsigned long long)n_raw, write, c->md.part.p);
        k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->md.junk.p, ptiles, c->md.stat.d + MD_ST_JUNK, c->md.part.p, 2, 1, c->md.stat.d + MD_ST_DUP_PAIRS);
    }
    if (n_ends) {
        k_md_flag_ends<<<etiles, MD_THREADS, 0, c->stream>>>(es.k[ew].p, es.v[ew].p, (uint32_t)n_ends, sv.rec, sv.dst_off, sv.tile, (uint32_t)n, (unsigned long long)n_raw, write, c->md.part.p);
        k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->md.junk.p, etiles, c->md.stat.d + MD_ST_JUNK, c->md.part.p, 1, 1, c->md.stat.d + MD_ST_DUP_FRAGS);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->md.ev[9], c->stream));
    if (write && n_ends) {                                        // bytes of the array changed: as behind dg_bam_sort_finish, no block of it has been compressed, and no track covers it
        bs_array_changed(c);
    }
    HIPCHK(c->md.stat.fetch(c->stream));
    HIPCHK(wait_stream(c));                                       // the third wait: the counts
    float t[9];
    for (int k = 0; k < 9; k++) t[k] = c->md.ev.ms(k, k + 1);
    c->md.ms[0] = t[0]; c->md.ms[1] = t[2]; c->md.ms[2] = t[6]; c->md.ms[3] = t[7]; c->md.ms[4] = t[8]; c->md.ms[5] = t[3] + t[5];
    float total = 0.f;
    for (float m : c->md.ms) total += m;
    if (device_ms) *device_ms = total;
    const uint64_t dup_pairs = c->md.stat.h[MD_ST_DUP_PAIRS], dup_frags = c->md.stat.h[MD_ST_DUP_FRAGS];
    if (stats) {
        stats[0] = n_examined; stats[1] = n_pairs; stats[2] = n_examined - 2 * n_pairs; stats[3] = dup_pairs; stats[4] = dup_frags; stats[5] = n_crowded;
        stats[6] = 2 * dup_pairs + dup_frags; stats[7] = c->md.stat.h[MD_ST_FAMILY];
    }
    return DG_OK;
}

extern "C" int dg_bam_markdup_device_ms(dg_ctx *c, float ms[6], int *n_passes)
{
    if (!c || !ms) return DG_ERR_ARG;
    for (int k = 0; k < 6; k++) ms[k] = c->md.ms[k];
    if (n_passes) *n_passes = c->md.passes;
    return DG_OK;
}

// ------------------------------------------------------------------------------------------
// UMI-aware duplicate marking of the sorted array (dg_umidup.h): dg_markdup.h's record rules, mate search and lists; U as one more sort key; groups, families,
// clusters and the flag writes are this stage's own kernels
// ------------------------------------------------------------------------------------------
extern "C" int dg_bam_markdup_umi_granules(int out[4])
{
    if (!out) return DG_ERR_ARG;
    out[0] = MD_THREADS; out[1] = RS_TILE; out[2] = MD_CROWD; out[3] = UD_FAMILY;
    return DG_OK;
}

// One sorted list (pairs: ends = 0, keys = lo; ends: ends = 1, keys = E) from its heads to its flags.  st: the list's UD_L_* words on the device; ev0: the first
// of its three events, which follow the event behind whatever ran in front of it
static int ud_verdicts(dg_ctx *c, const char *fn, const BsView &sv, const uint64_t *keys, const int64_t *vals, uint32_t n_items, int ends, uint32_t max_edit, int write,
                       unsigned long long *st, int ev0)
{
    UdState &u = c->ud;
    const uint32_t n = (uint32_t)sv.n, tiles = (n_items + MD_THREADS - 1) / MD_THREADS, wtiles = std::min<uint32_t>(tiles, 4u * (uint32_t)std::max(c->n_cu, 1));      // k_ud_cluster: 4 waves per workgroup, a few workgroups per CU at the most; a wave strides over the work list
    BS_ENSURE(u.mark, n_items, "the items' marks"); BS_ENSURE(u.grp_of, n_items, "the items' groups"); BS_ENSURE(u.gpos, (size_t)n_items + 1, "the groups' places");
    BS_ENSURE(u.ffirst, (size_t)n_items + 1, "the families' first groups"); BS_ENSURE(u.win, n_items, "the groups' winners"); BS_ENSURE(u.woff, n_items, "the families' offsets");
    BS_ENSURE(u.wl, (size_t)n_items / 2 + 1, "the work list"); BS_ENSURE(u.tile_h, (size_t)tiles + 1, "the per-workgroup sums"); BS_ENSURE(u.tile_w, (size_t)tiles + 1, "the per-workgroup sums");
    k_ud_heads<<<tiles, MD_THREADS, 0, c->stream>>>(keys, vals, n_items, ends, c->md.E.p, c->md.mate.p, u.U.p, u.mark.p, u.tile_h.p);
    k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(u.tile_h.p, tiles, st + UD_L_HEADS, nullptr, 0, 0, nullptr);
    k_ud_groups<<<tiles, MD_THREADS, 0, c->stream>>>(u.mark.p, u.tile_h.p, n_items, u.grp_of.p, u.gpos.p, u.ffirst.p, u.win.p);
    k_ud_fams<<<tiles, MD_THREADS, 0, c->stream>>>(u.ffirst.p, st + UD_L_HEADS, n_items, max_edit, u.woff.p, u.tile_w.p, u.part.p);
    k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(u.tile_w.p, tiles, st + UD_L_WORK, u.part.p, 2, 2, st + UD_L_MULTI);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(u.ev[ev0 + 0], c->stream));
    if (max_edit) {
        k_ud_worklist<<<tiles, MD_THREADS, 0, c->stream>>>(u.woff.p, u.tile_w.p, n_items, u.wl.p);
        k_ud_cluster<<<wtiles, MD_THREADS, 0, c->stream>>>(u.wl.p, st + UD_L_WORK, u.ffirst.p, u.gpos.p, vals, n_items, ends, u.U.p, c->md.score.p, c->md.mate.p, n, u.win.p, u.part.p);
        k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->md.junk.p, wtiles, c->ud.stat.d + UD_ST_JUNK, u.part.p, 2, 1, st + UD_L_ABSORBED);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(u.ev[ev0 + 1], c->stream));
    k_ud_flag<<<tiles, MD_THREADS, 0, c->stream>>>(vals, n_items, ends, u.grp_of.p, u.gpos.p, u.win.p, c->md.mate.p, sv.rec, sv.dst_off, sv.tile, n, (unsigned long long)sv.n_raw, write, u.part.p);
    k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->md.junk.p, tiles, c->ud.stat.d + UD_ST_JUNK, u.part.p, 2, 1, st + UD_L_DUP);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(u.ev[ev0 + 2], c->stream));
    return DG_OK;
}

extern "C" int dg_bam_markdup_umi_finish(dg_ctx *c, const dg_umi_rules *rules, uint32_t flags, uint64_t stats[12], float *device_ms)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_bam_markdup_umi_finish";
    if (device_ms) *device_ms = 0.f;
    if (stats) for (int k = 0; k < 12; k++) stats[k] = 0;
    UdState &u = c->ud;
    u.passes = 0;
    for (float &m : u.ms) m = 0.f;
    BsView sv;
    { const int rc = bs_view(c, fn, sv); if (rc) return rc; }
    if (flags & ~DG_MD_COUNT_ONLY) { snprintf(c->err, 512, "%s: flags 0x%x hold a bit that is not DG_MD_COUNT_ONLY", fn, flags); return DG_ERR_ARG; }
    if (!rules) { snprintf(c->err, 512, "%s: no rules", fn); return DG_ERR_ARG; }
    if (rules->flags) { snprintf(c->err, 512, "%s: rules->flags 0x%x: no bit is defined", fn, rules->flags); return DG_ERR_ARG; }
    if (rules->max_edit > 1u) { snprintf(c->err, 512, "%s: max_edit %u: 0 (exact) or 1", fn, rules->max_edit); return DG_ERR_ARG; }
    if (rules->sep == 0) { snprintf(c->err, 512, "%s: the separator is the NUL byte", fn); return DG_ERR_ARG; }
    const int write = (flags & DG_MD_COUNT_ONLY) ? 0 : 1;
    const uint32_t max_edit = rules->max_edit;
    HIPCHK(c->md.ready()); HIPCHK(u.ready());
    const size_t n = sv.n, n_raw = sv.n_raw;
    const int n_chr = sv.n_chr, hash_bits = c->md.hash_bits;
    if (n_chr < 1) { snprintf(c->err, 512, "%s: %d chromosomes", fn, n_chr); return DG_ERR_ARG; }
    if (!n) return DG_OK;
    const uint32_t tiles = (uint32_t)((n + MD_THREADS - 1) / MD_THREADS);
    BS_ENSURE(c->md.E, n, "the records' end keys"); BS_ENSURE(c->md.h, n, "the names' hashes"); BS_ENSURE(c->md.score, n, "the records' scores"); BS_ENSURE(c->md.mate, n, "the records' partners");
    BS_ENSURE(c->md.cand_off, n, "the candidates' offsets"); BS_ENSURE(c->md.cnt_off, n, "the pairs' and ends' offsets"); BS_ENSURE(u.U, n, "the records' UMIs");
    BS_ENSURE(c->md.tile, (size_t)tiles + 1, "the per-workgroup sums"); BS_ENSURE(c->md.junk, (size_t)tiles + 1, "the per-workgroup sums"); BS_ENSURE(c->md.part, 2 * (size_t)tiles, "the per-workgroup values");
    BS_ENSURE(u.part, 4 * (size_t)tiles + 4, "the per-workgroup values");
    HIPCHK(hipMemsetAsync(u.stat.d, 0, UD_ST_WORDS * 8, c->stream));
    HIPCHK(hipMemsetAsync(c->md.junk.p, 0, ((size_t)tiles + 1) * 8, c->stream));
    HIPCHK(hipEventRecord(u.ev[0], c->stream));
    k_ud_rec<<<tiles, MD_THREADS, 0, c->stream>>>(sv.rec, sv.dst_off, sv.tile, (uint32_t)n, (unsigned long long)n_raw, n_chr, hash_bits, (unsigned char)rules->sep, c->md.E.p, c->md.h.p, u.U.p,
                                                  c->md.score.p, c->md.mate.p, c->md.cand_off.p, c->md.tile.p, u.part.p);
    k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->md.tile.p, tiles, u.stat.d + UD_ST_CAND, u.part.p, 4, 2, u.stat.d + UD_ST_EXAMINED);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(u.ev[1], c->stream));
    HIPCHK(u.stat.fetch(c->stream));
    HIPCHK(wait_stream(c));                                       // the first wait: how many candidates, what was out of range, and the largest U
    if (u.stat.h[UD_ST_NBAD]) {
        snprintf(c->err, 512, "%s: record %llu of the sorted array has an unclipped 5' end outside [-2^31, 3 * 2^31): an end key cannot hold it; nothing was written", fn, ~u.stat.h[UD_ST_NBAD]);
        return DG_ERR_RANGE;
    }
    const size_t n_cand = (size_t)u.stat.h[UD_ST_CAND], n_examined = (size_t)u.stat.h[UD_ST_EXAMINED], n_umi = (size_t)u.stat.h[UD_ST_WITH_UMI];
    const int umi_bits = ud_umi_bits(u.stat.h[UD_ST_UMAX]);
    if (n_cand > n || n_examined > n || n_umi > n_examined) { snprintf(c->err, 512, "%s: %zu candidates, %zu examined records and %zu with a UMI of %zu", fn, n_cand, n_examined, n_umi, n); return DG_ERR_INTERNAL; }
    const uint32_t ctiles = (uint32_t)((n_cand + MD_THREADS - 1) / MD_THREADS);
    SortBufs &ps = c->md.sort, &es = c->md.esort;          // candidates, then pairs / ends
    int which = 0;
    if (n_cand) {
        for (int k = 0; k < 2; k++) { BS_ENSURE(ps.k[k], n_cand, "the sorter's keys"); BS_ENSURE(ps.v[k], n_cand, "the sorter's values"); }
        BS_ENSURE_SORT(ps, (uint32_t)n_cand);
    }
    HIPCHK(hipEventRecord(u.ev[2], c->stream));
    if (n_cand) {
        k_md_compact<<<tiles, MD_THREADS, 0, c->stream>>>(c->md.cand_off.p, c->md.tile.p, c->md.h.p, (uint32_t)n, (uint32_t)n_cand, ps.k[0].p, ps.v[0].p);
        { const int rc = ps.sort(c, (uint32_t)n_cand, hash_bits, which); if (rc) return rc; }
        u.passes += (hash_bits + 3) / 4;
        k_md_mate<<<ctiles, MD_THREADS, 0, c->stream>>>(ps.k[which].p, ps.v[which].p, (uint32_t)n_cand, (uint32_t)n, sv.rec, sv.dst_off, sv.tile, c->md.mate.p, c->md.part.p);
        k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->md.junk.p, ctiles, u.stat.d + UD_ST_JUNK, c->md.part.p, 1, 1, u.stat.d + UD_ST_CROWDED);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(u.ev[3], c->stream));
    k_md_count<<<tiles, MD_THREADS, 0, c->stream>>>(c->md.mate.p, (uint32_t)n, c->md.cnt_off.p, c->md.tile.p);
    k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->md.tile.p, tiles, u.stat.d + UD_ST_COUNTS, nullptr, 0, 0, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(u.ev[4], c->stream));
    HIPCHK(u.stat.fetch(c->stream));
    HIPCHK(wait_stream(c));                                       // the second wait: how many pairs and ends
    const size_t n_pairs = (size_t)(u.stat.h[UD_ST_COUNTS] >> 32), n_ends = (size_t)(uint32_t)u.stat.h[UD_ST_COUNTS], n_crowded = (size_t)u.stat.h[UD_ST_CROWDED];
    if (2 * n_pairs > n_cand || n_ends != n_examined) { snprintf(c->err, 512, "%s: %zu pairs of %zu candidates, %zu ends of %zu examined records", fn, n_pairs, n_cand, n_ends, n_examined); return DG_ERR_INTERNAL; }
    const uint32_t ptiles = (uint32_t)((n_pairs + MD_THREADS - 1) / MD_THREADS), etiles = (uint32_t)((n_ends + MD_THREADS - 1) / MD_THREADS);
    if (n_ends) {
        for (int k = 0; k < 2; k++) { BS_ENSURE(es.k[k], n_ends, "the ends' keys"); BS_ENSURE(es.v[k], n_ends, "the ends' values"); }
        BS_ENSURE_SORT(es, (uint32_t)n_ends);
    }
    const int e_bits = md_e_bits(n_chr);
    int pw = 0, ew = 0;
    HIPCHK(hipEventRecord(u.ev[5], c->stream));
    if (n_ends) k_md_emit<<<tiles, MD_THREADS, 0, c->stream>>>(c->md.mate.p, c->md.score.p, c->md.cnt_off.p, c->md.tile.p, (uint32_t)n, (uint32_t)n_pairs, (uint32_t)n_ends, ps.k[0].p, ps.v[0].p, es.k[0].p, es.v[0].p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(u.ev[6], c->stream));
    if (n_pairs) {                                                // (lo, hi, U, score descending, rep)
        { const int rc = ps.sort(c, (uint32_t)n_pairs, MD_SCORE_BITS, pw); if (rc) return rc; }
        if (umi_bits) {
            k_ud_rekey_u<<<ptiles, MD_THREADS, 0, c->stream>>>(ps.k[pw].p, ps.v[pw].p, (uint32_t)n_pairs, u.U.p, (uint32_t)n);
            { const int rc = ps.sort(c, (uint32_t)n_pairs, umi_bits, pw); if (rc) return rc; }
        }
        k_md_rekey<<<ptiles, MD_THREADS, 0, c->stream>>>(ps.k[pw].p, ps.v[pw].p, (uint32_t)n_pairs, 0, c->md.E.p, c->md.mate.p, (uint32_t)n);
        { const int rc = ps.sort(c, (uint32_t)n_pairs, e_bits, pw); if (rc) return rc; }
        k_md_rekey<<<ptiles, MD_THREADS, 0, c->stream>>>(ps.k[pw].p, ps.v[pw].p, (uint32_t)n_pairs, 1, c->md.E.p, c->md.mate.p, (uint32_t)n);
        { const int rc = ps.sort(c, (uint32_t)n_pairs, e_bits, pw); if (rc) return rc; }
        u.passes += (MD_SCORE_BITS + 3) / 4 + (umi_bits + 3) / 4 + 2 * ((e_bits + 3) / 4);
    }
    HIPCHK(hipEventRecord(u.ev[7], c->stream));
    if (n_ends) {                                                 // (E, U, paired first, score descending, index)
        { const int rc = es.sort(c, (uint32_t)n_ends, MD_SCORE_BITS, ew); if (rc) return rc; }
        if (umi_bits) {
            k_ud_rekey_u<<<etiles, MD_THREADS, 0, c->stream>>>(es.k[ew].p, es.v[ew].p, (uint32_t)n_ends, u.U.p, (uint32_t)n);
            { const int rc = es.sort(c, (uint32_t)n_ends, umi_bits, ew); if (rc) return rc; }
        }
        k_md_rekey<<<etiles, MD_THREADS, 0, c->stream>>>(es.k[ew].p, es.v[ew].p, (uint32_t)n_ends, 2, c->md.E.p, c->md.mate.p, (uint32_t)n);
        { const int rc = es.sort(c, (uint32_t)n_ends, e_bits, ew); if (rc) return rc; }
        u.passes += (MD_SCORE_BITS + 3) / 4 + (umi_bits + 3) / 4 + (e_bits + 3) / 4;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(u.ev[8], c->stream));
    // (the events of a list that is empty are recorded all the same: the stages' times stay defined)
    if (n_pairs) { const int rc = ud_verdicts(c, fn, sv, ps.k[pw].p, ps.v[pw].p, (uint32_t)n_pairs, 0, max_edit, write, u.stat.d + UD_ST_PAIRS, 9); if (rc) return rc; }
    else for (int k = 9; k < 12; k++) HIPCHK(hipEventRecord(u.ev[k], c->stream));
    if (n_ends) { const int rc = ud_verdicts(c, fn, sv, es.k[ew].p, es.v[ew].p, (uint32_t)n_ends, 1, max_edit, write, u.stat.d + UD_ST_ENDS, 12); if (rc) return rc; }
    else for (int k = 12; k < 15; k++) HIPCHK(hipEventRecord(u.ev[k], c->stream));
    if (write && n_ends) bs_array_changed(c);                     // bytes of the array changed: as behind dg_bam_markdup_finish
    HIPCHK(u.stat.fetch(c->stream));
    HIPCHK(wait_stream(c));                                       // the third wait: the counts
    float t[14];
    for (int k = 0; k < 14; k++) t[k] = u.ev.ms(k, k + 1);
    u.ms[0] = t[0]; u.ms[1] = t[2]; u.ms[2] = t[6]; u.ms[3] = t[7]; u.ms[4] = t[8] + t[11]; u.ms[5] = t[9] + t[12]; u.ms[6] = t[10] + t[13]; u.ms[7] = t[3] + t[5];
    float total = 0.f;
    for (float m : u.ms) total += m;
    if (device_ms) *device_ms = total;
    const unsigned long long *P = u.stat.h + UD_ST_PAIRS, *Q = u.stat.h + UD_ST_ENDS;
    const uint64_t dup_pairs = P[UD_L_DUP], dup_frags = Q[UD_L_DUP];
    if (stats) {
        stats[0] = n_examined; stats[1] = n_pairs; stats[2] = n_examined - 2 * n_pairs; stats[3] = dup_pairs; stats[4] = dup_frags; stats[5] = n_crowded;
        stats[6] = 2 * dup_pairs + dup_frags; stats[7] = P[UD_L_CLUSTER_MAX] > P[UD_L_GROUP_MAX] ? P[UD_L_CLUSTER_MAX] : P[UD_L_GROUP_MAX];
        stats[8] = n_umi; stats[9] = P[UD_L_MULTI]; stats[10] = P[UD_L_ABSORBED] + Q[UD_L_ABSORBED]; stats[11] = P[UD_L_CROWDED] + Q[UD_L_CROWDED];
    }
    return DG_OK;
}

extern "C" int dg_bam_markdup_umi_device_ms(dg_ctx *c, float ms[8], int *n_passes)
{
    if (!c || !ms) return DG_ERR_ARG;
    for (int k = 0; k < 8; k++) ms[k] = c->ud.ms[k];
    if (n_passes) *n_passes = c->ud.passes;
    return DG_OK;
}

// ------------------------------------------------------------------------------------------
// MD / NM / ts on the sorted array (dg_tags.h): the one stage that changes the records' sizes: new lengths, a scan, a rewrite into a second array, which then
// takes the sorted array's place in everything bs_view hands out
// ------------------------------------------------------------------------------------------
extern "C" int dg_bam_tags_granules(int out[3])
{
    if (!out) return DG_ERR_ARG;
    out[0] = TG_WG; out[1] = TG_LANES; out[2] = PU_STEP;
    return DG_OK;
}

template <typename T> static void tg_swap(DBuf<T> &a, DBuf<T> &b) { std::swap(a.p, b.p); std::swap(a.cap, b.cap); }

extern "C" int dg_bam_tags_finish(dg_ctx *c, uint32_t flags, size_t *n_raw_out, uint64_t stats[8], float *device_ms)
{
    if (!c) return DG_ERR_ARG;
    const char *fn = "dg_bam_tags_finish";
    if (n_raw_out) *n_raw_out = 0;
    if (device_ms) *device_ms = 0.f;
    if (stats) for (int k = 0; k < 8; k++) stats[k] = 0;
    c->tg.ms[0] = c->tg.ms[1] = c->tg.write_ms[0] = c->tg.write_ms[1] = 0.f;
    if (flags == 0u || (flags & ~TG_ALL)) { snprintf(c->err, 512, "%s: flags 0x%x are not a non-empty set of DG_TAG_MD, DG_TAG_NM, DG_TAG_TS", fn, flags); return DG_ERR_ARG; }
    BsView sv;
    { const int rc = bs_view(c, fn, sv); if (rc) return rc; }
    HIPCHK(c->tg.ready());
    const size_t n = sv.n, n_raw = sv.n_raw;
    if (sv.n_chr < 1) { snprintf(c->err, 512, "%s: %d chromosomes", fn, sv.n_chr); return DG_ERR_ARG; }
    if (!n) return DG_OK;
    const DIndex ix = c->ix;
    const uint32_t tiles = (uint32_t)((n + TG_WG - 1) / TG_WG);
    BS_ENSURE(c->tg.off, n, "the records' new places"); BS_ENSURE(c->tg.tile, (size_t)tiles + 1, "the per-workgroup sums"); BS_ENSURE(c->tg.junk, (size_t)tiles + 1, "the per-workgroup scratch");
    BS_ENSURE(c->tg.part, (size_t)CV_PLANES * tiles, "the per-workgroup values"); BS_ENSURE(c->tg.part2, (size_t)tiles, "the per-workgroup values");
    HIPCHK(hipMemsetAsync(c->tg.stat.d, 0, TG_ST_WORDS * 8, c->stream));
    HIPCHK(hipMemsetAsync(c->tg.junk.p, 0, ((size_t)tiles + 1) * 8, c->stream));
    HIPCHK(hipEventRecord(c->tg.ev[0], c->stream));
    k_tg_len<<<tiles, TG_WG, 0, c->stream>>>(sv.rec, sv.dst_off, sv.tile, (uint32_t)n, (unsigned long long)n_raw, ix, flags, c->tg.off.p, c->tg.tile.p, c->tg.part.p, c->tg.part2.p);
    k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->tg.tile.p, tiles, c->tg.stat.d + TG_ST_BYTES, c->tg.part.p, 5, 5, c->tg.stat.d + TG_ST_RECS);
    k_cv_top<<<1, CV_THREADS, 0, c->stream>>>(c->tg.junk.p, tiles, c->tg.stat.d + TG_ST_JUNK, c->tg.part2.p, 1, 1, c->tg.stat.d + TG_ST_NO_TS);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->tg.ev[1], c->stream));
    HIPCHK(c->tg.stat.fetch(c->stream));
    HIPCHK(wait_stream(c));                                       // the one wait in front of the rewrite: the new array's size
    const unsigned long long *st = c->tg.stat.h;
    const size_t bytes = (size_t)st[TG_ST_BYTES];
    const unsigned long long rewritten = (uint32_t)st[TG_ST_RECS], not_eligible = st[TG_ST_RECS] >> 32, aux_bad = (uint32_t)st[TG_ST_AUX_TS];
    if (rewritten + not_eligible + aux_bad != n) { snprintf(c->err, 512, "%s: %llu records rewritten and %llu + %llu copied of %zu", fn, rewritten, not_eligible, aux_bad, n); return DG_ERR_INTERNAL; }
    BS_ENSURE(c->tg.sorted, bytes + 8, "the tagged records");
    HIPCHK(hipEventRecord(c->tg.ev[2], c->stream));
    k_tg_tail<<<tiles, TG_WG, 0, c->stream>>>(sv.rec, sv.dst_off, sv.tile, (uint32_t)n, (unsigned long long)n_raw, ix, flags, c->tg.off.p, c->tg.tile.p, (unsigned long long)bytes, c->tg.sorted.p);
    HIPCHK(hipEventRecord(c->tg.ev[4], c->stream));
    k_tg_copy<<<(unsigned)((n + TG_WG / TG_LANES - 1) / (TG_WG / TG_LANES)), TG_WG, 0, c->stream>>>(sv.rec, sv.dst_off, sv.tile, (uint32_t)n, (unsigned long long)n_raw, ix, flags, c->tg.off.p,
                                                                                                    c->tg.tile.p, (unsigned long long)bytes, c->tg.sorted.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->tg.ev[3], c->stream));
    HIPCHK(wait_stream(c));
    // the new array takes the old one's place: its bytes, every record's place inside its tile, the tiles' sums, the size
    tg_swap(c->bs.sorted, c->tg.sorted); tg_swap(c->bs.sort.k[c->bs.fin_which ^ 1], c->tg.off); tg_swap(c->bs.tile, c->tg.tile);
    c->bs.fin_bytes = bytes;
    bs_array_changed(c);
    c->tg.ms[0] = c->tg.ev.ms(0, 1); c->tg.ms[1] = c->tg.ev.ms(2, 3);
    c->tg.write_ms[0] = c->tg.ev.ms(2, 4); c->tg.write_ms[1] = c->tg.ev.ms(4, 3);
    if (n_raw_out) *n_raw_out = bytes;
    if (device_ms) *device_ms = c->tg.ms[0] + c->tg.ms[1];
    if (stats) {
        stats[0] = rewritten; stats[1] = not_eligible; stats[2] = aux_bad; stats[3] = st[TG_ST_REMOVED]; stats[4] = st[TG_ST_MISM]; stats[5] = st[TG_ST_INDEL];
        stats[6] = st[TG_ST_AUX_TS] >> 32; stats[7] = st[TG_ST_NO_TS];
    }
    return DG_OK;
}

extern "C" int dg_bam_tags_device_ms(dg_ctx *c, float ms[2])
{
    if (!c || !ms) return DG_ERR_ARG;
    ms[0] = c->tg.ms[0]; ms[1] = c->tg.ms[1];
    return DG_OK;
}

// a probe's hook (not in the public header): the write pass by kernel: [0] k_tg_tail, [1] k_tg_copy
extern "C" int dg_bam_tags_write_ms(dg_ctx *c, float ms[2])
{
    if (!c || !ms) return DG_ERR_ARG;
    ms[0] = c->tg.write_ms[0]; ms[1] = c->tg.write_ms[1];
    return DG_OK;
}

// ---- roofline calibration (not in the public header): random 64-byte block reads over the resident
// Occ array, the access pattern of k_seed / k_locate without any of their arithmetic.
// dependent = 1: the next block index depends on the loaded data (a chain per lane, like an FM walk);
// dependent = 0: indices are a pure function of (lane, iteration).
__global__ void __launch_bounds__(256)
k_rand_blocks(const uint4 *__restrict__ bwt, uint64_t n_blocks, int iters, int dependent, uint32_t *__restrict__ sink)
{
    uint64_t x = (uint64_t)(blockIdx.x * blockDim.x + threadIdx.x) * 0x9E3779B97F4A7C15ull + 12345;
    uint32_t acc = 0;
    for (int it = 0; it < iters; it++) {
        x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
        const uint4 *p = bwt + ((x % n_blocks) << 2);
        const uint4 a = p[0], b = p[1], cc = p[2], d = p[3];
        const uint32_t v = a.x ^ b.y ^ cc.z ^ d.w;
        acc += v;
        if (dependent) x += v;
    }
    if (acc == 0x12345678u) sink[0] = acc;
}
// quad-cooperative variant: the 4 lanes of a quad fetch the four 16-byte pieces of ONE block with one
// instruction (one 64-byte line per quad per load instruction instead of four instructions per lane)
__global__ void __launch_bounds__(256)
k_rand_blocks_quad(const uint4 *__restrict__ bwt, uint64_t n_blocks, int iters, int dependent, uint32_t *__restrict__ sink)
{
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t x = (uint64_t)(tid >> 2) * 0x9E3779B97F4A7C15ull + 12345;
    uint32_t acc = 0;
    for (int it = 0; it < iters; it++) {
        x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
        const uint4 a = bwt[((x % n_blocks) << 2) + (tid & 3)];
        uint32_t v = a.x ^ a.y ^ a.z ^ a.w;
        v ^= __shfl_xor((int)v, 1, 64); v ^= __shfl_xor((int)v, 2, 64);      // every lane of the quad sees the whole block
        acc += v;
        if (dependent) x += v;
    }
    if (acc == 0x12345678u) sink[0] = acc;
}

extern "C" int dg_debug_random_blocks(dg_ctx *c, int iters, int dependent, int waves_per_cu, float *ms, unsigned long long *n_loads)
{
    if (!c) return DG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    const uint64_t n_blocks = (c->ix.seq_len + 127) / 128;
    const unsigned blocks = (unsigned)(c->n_cu * waves_per_cu / 4);
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    const int quad = dependent >> 1; dependent &= 1;
    if (quad) k_rand_blocks_quad<<<blocks, 256, 0, c->stream>>>(c->ix.bwt, n_blocks, 4, dependent, (uint32_t *)c->d_err);
    else k_rand_blocks<<<blocks, 256, 0, c->stream>>>(c->ix.bwt, n_blocks, 4, dependent, (uint32_t *)c->d_err);   // warm
    HIPCHK(hipEventRecord(e0, c->stream));
    if (quad) k_rand_blocks_quad<<<blocks, 256, 0, c->stream>>>(c->ix.bwt, n_blocks, iters, dependent, (uint32_t *)c->d_err);
    else k_rand_blocks<<<blocks, 256, 0, c->stream>>>(c->ix.bwt, n_blocks, iters, dependent, (uint32_t *)c->d_err);
    HIPCHK(hipEventRecord(e1, c->stream));
    HIPCHK(hipEventSynchronize(e1));
    HIPCHK(hipEventElapsedTime(ms, e0, e1));
    *n_loads = (unsigned long long)blocks * (quad ? 64ull : 256ull) * (unsigned long long)iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return DG_OK;
}

// debugging aid (not in the public header): the re-seed job queue of the last run
extern "C" int dg_debug_jobs(dg_ctx *c, void *out, int cap)
{
    unsigned int n = c->h_tail ? c->h_tail->tops[TOP_JOBS] : 0u;       // (the device copy is zeroed by k_batch_end)
    if ((int)n > cap) n = (unsigned)cap;
    if (n && hipMemcpy(out, c->jobs.p, (size_t)n * sizeof(DJob), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int)n;
}

extern "C" int dg_last_timings(dg_ctx *c, const char **names, float *ms, int cap)
{
    if (!c) return 0;
    int k = c->n_t < cap ? c->n_t : cap;
    for (int i = 0; i < k; i++) { names[i] = c->tname[i]; ms[i] = c->tms[i]; }
    return k;
}

extern "C" int dg_last_counters(dg_ctx *c, uint64_t *out, int cap)
{
    if (!c) return 0;
    int k = CTR_R4_N < cap ? CTR_R4_N : cap;
    for (int i = 0; i < k; i++) out[i] = c->counters[i];
    // [36] units that took the general path, [37] units chained by a wave each, [38] times the batch was enqueued, [39] / [40] re-runs of this context so far: capacity grown / scan not completed (> 1: a buffer grew)
    const uint64_t extra[5] = { c->h_tail ? c->h_tail->sizes.n_slow_units : 0u, c->h_tail ? c->h_tail->tops[TOP_HEAVY_UNITS] : 0u, (uint64_t)c->runs_of_last_batch,
                                c->reruns_capacity, c->reruns_scan };
    for (int i = 0; i < 5 && k < cap; i++) out[k++] = extra[i];
    for (int i = CTR_R4_N; i < CTR_N && k < cap; i++) out[k++] = c->counters[i];        // [41] windows scanned again whole, [42] (window, chunk) items of k_reseed
    return k;
}

// diagnostic: the per-tile trace of one of the last run's single-pass scans (dg_scan.h, SCAN_TRACE_WORDS u64 per tile: epoch << 32 | HW_ID, wall clock at the
// ticket, at the publication of the tile's own totals, XCC_ID << 56 | wall clock at the publication of its prefix), for tests/probes/kpair_wait.py:
// how long does a workgroup of k_pair work before its look-back, and how long does the look-back wait?  which: 0 = k_seed_offsets, 1 = k_pair, 2 = k_emit_slow
extern "C" int dg_debug_scan_trace(dg_ctx *c, int which, uint64_t *out, size_t cap_tiles, size_t *n_tiles, double *ticks_per_ms)
{
    if (!c || !out || !n_tiles || which < 0 || which > 2) return DG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    const int n = c->n_reads, paired = (c->pr.paired && (n % 2 == 0)) ? 1 : 0, n_units = paired ? n / 2 : n;
    const size_t ts = scan_tiles_seed(n), tp = scan_tiles_pair(n_units), te = (size_t)(2 * n_units + 255) / 256 + 1;
    const size_t first = which == 0 ? 0 : (which == 1 ? ts : ts + tp), cnt = (which == 0 ? ts : (which == 1 ? tp : te)) - 1;
    *n_tiles = cnt;
    if (ticks_per_ms) *ticks_per_ms = (double)c->wall_khz;
    if (!c->scan_trace.p || cnt > cap_tiles) return cnt > cap_tiles ? DG_ERR_CAPACITY : DG_ERR_ARG;
    HIPCHK(hipMemcpy(out, c->scan_trace.p + SCAN_TRACE_WORDS * first, cnt * SCAN_TRACE_WORDS * 8, hipMemcpyDeviceToHost));
    return DG_OK;
}

// ---- the index builder's sorter (dg_sort.h): stable radix sort of n (key, value) pairs in device memory, ascending by the low
// key_bits bits of the key.  keys/vals hold the input and the result; *_tmp are scratch of the same size.  Runs on the NULL
// stream of `device` (so it is ordered with a caller that uses the default stream, e.g. torch) and returns when it is done.
extern "C" int dg_sort_pairs(int device, uint64_t *keys, int64_t *vals, uint64_t *keys_tmp, int64_t *vals_tmp, size_t n, int key_bits)
{
    dg_ctx *c = nullptr;                                   // (HIPCHK reports through the init error string)
    if (!keys || !vals || !keys_tmp || !vals_tmp || key_bits < 1 || key_bits > 64 || n >= 0xFFFFF000ull) return DG_ERR_ARG;
    HIPCHK(hipSetDevice(device));
    if (n < 2) return DG_OK;
    uint32_t *hist = nullptr, *sums = nullptr;
    HIPCHK(hipMalloc((void **)&hist, rs_hist_words((uint32_t)n) * 4));
    if (hipMalloc((void **)&sums, rs_sums_words((uint32_t)n) * 4) != hipSuccess) { (void)hipFree(hist); return DG_ERR_HIP; }
    uint64_t *const k2[2] = {keys, keys_tmp}; int64_t *const v2[2] = {vals, vals_tmp};
    int which = 0;
    hipError_t e = rs_sort_passes(0, k2, v2, hist, sums, (uint32_t)n, key_bits, which);
    if (e == hipSuccess && which) {
        e = hipMemcpyAsync(keys, keys_tmp, n * 8, hipMemcpyDeviceToDevice, 0);
        if (e == hipSuccess) e = hipMemcpyAsync(vals, vals_tmp, n * 8, hipMemcpyDeviceToDevice, 0);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(0);
    (void)hipFree(hist); (void)hipFree(sums);
    if (e != hipSuccess) return fail(nullptr, DG_ERR_HIP, "dg_sort_pairs", e);
    return DG_OK;
}

// ---- stage probes ----
extern "C" int dg_probe_sort_passes(int device, uint64_t *keys, int64_t *vals, uint64_t *keys_tmp, int64_t *vals_tmp, size_t n, int key_bits, float *ms, int *in_tmp)
{
    dg_ctx *c = nullptr;                                   // (HIPCHK reports through the init error string)
    if (!keys || !vals || !keys_tmp || !vals_tmp || !ms || key_bits < 1 || key_bits > 64 || n < 2 || n >= 0xFFFFF000ull) return DG_ERR_ARG;
    HIPCHK(hipSetDevice(device));
    uint32_t *hist = nullptr, *sums = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipMalloc((void **)&hist, rs_hist_words((uint32_t)n) * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&sums, rs_sums_words((uint32_t)n) * 4);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    uint64_t *const k2[2] = {keys, keys_tmp}; int64_t *const v2[2] = {vals, vals_tmp};
    int which = 0;
    if (e == hipSuccess) e = hipEventRecord(e0, 0);
    if (e == hipSuccess) e = rs_sort_passes(0, k2, v2, hist, sums, (uint32_t)n, key_bits, which);
    if (e == hipSuccess) e = hipEventRecord(e1, 0);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, e0, e1);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(hist); (void)hipFree(sums);
    if (in_tmp) *in_tmp = which;
    if (e != hipSuccess) return fail(nullptr, DG_ERR_HIP, "dg_probe_sort_passes", e);
    return DG_OK;
}

extern "C" int dg_probe_seeds(dg_ctx *c, int n_reads, const uint32_t *seq_off, const uint16_t *rlen, const char *seq,
                              uint32_t *seed_off, int32_t *rpos, int32_t *slen, int64_t *gpos, size_t cap, size_t *used)
{
    int rc = dg_batch_upload(c, n_reads, seq_off, rlen, seq);
    if (rc) return rc;
    const int n = n_reads;
    if (used) *used = 0;
    if (n == 0) return DG_OK;
    const int H = c->max_rlen / 16 + 1;
    uint32_t total = 0;
    for (int attempt = 0; ; attempt++) {
        c->n_t = 0;
        if ((rc = zero_batch_state(c, n, n))) return rc;
        if ((rc = enqueue_seeding(c, n, H, false, false))) return rc;
        // the production sorters, every read on its own (unpaired): k_chain_heavy for the long lists, k_pair (candidate stage
        // only, sorted seeds written back for every read) for the rest
        HIPCHK(c->ncand.ensure(n)); HIPCHK(c->rep_off.ensure((size_t)n + 1)); HIPCHK(c->reads_out.ensure(n));
        HIPCHK(c->heavy.ensure((size_t)n + 16)); HIPCHK(c->slow_units.ensure((size_t)n + 16)); HIPCHK(c->reports.ensure(16)); HIPCHK(c->cigfinal.ensure(16));
        HIPCHK(c->chain_picks.ensure(c->cap_seeds + 16)); HIPCHK(c->chain_todo.ensure((size_t)n + 16));
        k_chain_heavy<<<c->n_cu * 4, 64, 0, c->stream>>>(c->ix, c->pr, n, 0, c->rlen.p, c->seed_off.p, c->seeds.p, c->cands.p, c->ncand.p, c->heavy.p, c->d_tops + TOP_HEAVY_UNITS, c->chain_picks.p, c->chain_todo.p, c->d_ctr, c->d_err);
        k_chain_rules<<<c->n_cu * 4, 64, 0, c->stream>>>(0, c->seed_off.p, c->cands.p, c->ncand.p, c->heavy.p, c->d_tops + TOP_HEAVY_UNITS, c->chain_picks.p, c->chain_todo.p, c->d_err);
        const TileScan ts = make_tile_scan(c, scan_tiles_seed(n), c->d_tops + TOP_TICKET_PAIR, 2);
        k_pair<false><<<(unsigned)((n + PU_THREADS - 1) / PU_THREADS), PU_THREADS, 0, c->stream>>>(
            c->ix, c->pr, n, 0, 0, 1, c->seq.p, c->seq_off.p, c->enc.p, 1, c->rlen.p, c->seed_off.p, c->seeds.p, c->cands.p, c->ncand.p, c->rep_off.p,
            c->slow_units.p, c->reads_out.p, c->reports.p, c->cigfinal.p, 0xFFFFFFFFu, 0xFFFFFFFFu, ts, c->d_sizes, c->d_tops + TOP_CIG, c->d_ctr, c->d_err, CompactOut{nullptr, nullptr, nullptr, nullptr});
        HIPCHK(hipGetLastError());
        k_batch_end<<<1, 256, 0, c->stream>>>(c->d_sizes, c->d_err, c->d_tops, c->d_ctr, c->h_tail);
        HIPCHK(hipGetLastError());
        c->state_zeroed = true;
        HIPCHK(hipStreamSynchronize(c->stream));
        total = c->h_tail->sizes.total_seeds;
        if (c->h_tail->err == DG_E_SEEDS && attempt < 3) { c->cap_seeds = (size_t)total + total / 4 + 1024; continue; }
        if (c->h_tail->err) { snprintf(c->err, 512, "dg_probe_seeds: device status %d", c->h_tail->err); return DG_ERR_INTERNAL; }
        break;
    }
    if (used) *used = total;
    if (total > cap) return DG_ERR_CAPACITY;
    std::vector<SKey> h(total);
    HIPCHK(hipMemcpyAsync(seed_off, c->seed_off.p, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    if (total) HIPCHK(hipMemcpyAsync(h.data(), c->seeds.p, (size_t)total * sizeof(SKey), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < total; i++) { rpos[i] = sk_rpos(h[i]); slen[i] = sk_rlen(h[i]); gpos[i] = sk_gpos(h[i]); }
    return DG_OK;
}

// ---- nw_alignment probes: every form of nw_alignment.cpp:18-82 that runs in production, one pair per lane ----
// mode 0: the serial strip form d_nw (string path of d_process_pair)
__global__ void __launch_bounds__(64)
k_probe_nw(int n, const uint32_t *a_off, const uint32_t *b_off, const char *a, const char *b, const uint32_t *out_off,
           uint32_t *out_len, char *out_a, char *out_b, unsigned char *ws, const WSLayout L, const DIndex ix, const DParams pr)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    LaneCtx cx;
    cx.ix = &ix; cx.pr = &pr; cx.L = &L; cx.ws = ws + (size_t)i * L.stride; cx.seq = nullptr; cx.rlen = 0; cx.lds = nullptr;
    cx.n_nw = cx.nw_cells = cx.n_reseed = cx.reseed_w = 0;
    out_len[i] = (uint32_t)d_nw(cx, a + a_off[i], (int)(a_off[i + 1] - a_off[i]), b + b_off[i], (int)(b_off[i + 1] - b_off[i]), out_a + out_off[i], out_b + out_off[i]);
}
// mode 1: the register-strip form d_pair_nw (pairs up to PM_MAX x PM_MAX: strings as bytes in registers, traceback bits in
// the lane's LDS slice, result = a column list); the gapped strings are rebuilt from the column list
__global__ void __launch_bounds__(64)
k_probe_nw_strips(int n, const uint32_t *a_off, const uint32_t *b_off, const char *a, const char *b, const uint32_t *out_off,
                  uint32_t *out_len, char *out_a, char *out_b, const DIndex ix, const DParams pr)
{
    __shared__ uint32_t lds_pm[64 * PM_LDS_WORDS];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    LaneCtx cx;
    cx.ix = &ix; cx.pr = &pr; cx.L = nullptr; cx.ws = nullptr; cx.seq = nullptr; cx.rlen = 0; cx.lds = lds_pm + (threadIdx.x & 63) * PM_LDS_WORDS;
    cx.n_nw = cx.nw_cells = cx.n_reseed = cx.reseed_w = 0;
    const char *pa = a + a_off[i], *pb = b + b_off[i];
    const int m = (int)(a_off[i + 1] - a_off[i]), nn = (int)(b_off[i + 1] - b_off[i]);
    uint64_t w[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < m; k++) w[k >> 3] |= (uint64_t)(unsigned char)pa[k] << ((k & 7) << 3);
    for (int k = 0; k < nn; k++) w[3 + (k >> 3)] |= (uint64_t)(unsigned char)pb[k] << ((k & 7) << 3);
    PairStr ps; ps.A0 = w[0]; ps.A1 = w[1]; ps.A2 = w[2]; ps.B0 = w[3]; ps.B1 = w[4]; ps.B2 = w[5];
    ColList cl;
    d_pair_nw(cx, m, nn, ps, cl);
    char *oa = out_a + out_off[i], *ob = out_b + out_off[i];
    int x = 0, y = 0;
    for (int p_ = 0; p_ < cl.K; p_++) {
        const uint32_t ty = d_colcode(cl, p_) & 3u;
        oa[p_] = ty == 1 ? '-' : pa[x++];
        ob[p_] = ty == 2 ? '-' : pb[y++];
    }
    out_len[i] = (uint32_t)cl.K;
}
// modes 2 and 3: the wave-wide service d_nw_wave (8-lane groups up to 64 columns, the whole wave beyond; mode 3: the whole-wave
// form for every pair) + the owner's traceback d_tb_traceback.  The genome side comes from a pac (here: the b strings packed
// 2 bit/base), exactly as in k_report.
__global__ void __launch_bounds__(64)
k_probe_nw_wave(int n, int all_wide, const uint32_t *a_off, const uint32_t *b_off, const char *a, const uint32_t *out_off,
                uint32_t *out_len, char *out_a, char *out_b, unsigned char *ws, const WSLayout L, const DIndex ix, const DParams pr)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const bool has = i < n;
    LaneCtx cx;
    cx.ix = &ix; cx.pr = &pr; cx.L = &L; cx.ws = ws + (size_t)(has ? i : 0) * L.stride; cx.seq = nullptr; cx.rlen = 0; cx.lds = nullptr;
    cx.n_nw = cx.nw_cells = cx.n_reseed = cx.reseed_w = 0;
    const int m = has ? (int)(a_off[i + 1] - a_off[i]) : 0, nn = has ? (int)(b_off[i + 1] - b_off[i]) : 0;
    const unsigned char *pa = (const unsigned char *)a + (has ? a_off[i] : 0);
    const int64_t gPos = has ? (int64_t)b_off[i] : 0;
    d_nw_wave(cx, has, pa, m, gPos, nn, lane, all_wide != 0);
    if (has) {
        char *g = ws_str(cx, 0);
        d_ref_fill(ix, gPos, nn, g);
        out_len[i] = (uint32_t)d_tb_traceback(cx, (const char *)pa, m, g, nn, out_a + out_off[i], out_b + out_off[i]);
    }
}

struct DevTmp {                       // frees its device buffers on every return path
    std::vector<void *> ptrs;
    hipError_t alloc(void **p, size_t bytes) { hipError_t e = hipMalloc(p, bytes ? bytes : 16); if (e == hipSuccess) ptrs.push_back(*p); return e; }
    ~DevTmp() { for (void *p : ptrs) (void)hipFree(p); }
};

extern "C" int dg_probe_nw_mode(dg_ctx *c, int mode, int n, const uint32_t *a_off, const uint32_t *b_off, const char *a, const char *b,
                                uint32_t *out_off, uint32_t *out_len, char *out_a, char *out_b, size_t cap)
{
    if (!c || n < 0 || mode < 0 || mode > 3) return DG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (n == 0) return DG_OK;
    size_t tot = 0; int mx = 32;
    for (int i = 0; i < n; i++) {
        const int m = (int)(a_off[i + 1] - a_off[i]), nn = (int)(b_off[i + 1] - b_off[i]);
        out_off[i] = (uint32_t)tot; tot += (size_t)m + nn;
        if (m > mx) mx = m;
        if ((nn + 1) / 2 > mx) mx = (nn + 1) / 2;      // workspace bit matrix holds 2R+32 columns
        if (mode == 1 && (m > PM_MAX || nn > PM_MAX || m < 1 || nn < 1)) { snprintf(c->err, 512, "dg_probe_nw_mode 1: pair %d is not within %d x %d", i, PM_MAX, PM_MAX); return DG_ERR_ARG; }
    }
    if (tot > cap) return DG_ERR_CAPACITY;
    const size_t la = a_off[n], lb = b_off[n];
    std::vector<uint8_t> pac;
    if (mode >= 2) {                                   // the genome side as a pac (2 bit/base, first base on top): forward strand, then -- as every pac a kernel sees -- its reverse complement
        pac.assign(pac_both_bytes((int64_t)lb) + 4096, 0);
        for (size_t k = 0; k < lb; k++) {
            const uint8_t code = d_nt4((unsigned char)b[k]);
            if (code > 3) { snprintf(c->err, 512, "dg_probe_nw_mode %d: the genome side must be ACGT (RefSequence holds nothing else)", mode); return DG_ERR_ARG; }
            pac[k >> 2] |= (uint8_t)(code << ((~k & 3) << 1));
        }
        for (size_t q = lb / 4; q < pac_both_bytes((int64_t)lb); q++) pac[q] = d_pac_both_byte(pac.data(), (int64_t)lb, (int64_t)q);
    }
    const WSLayout L = make_ws_layout(mx);
    DevTmp tmp;
    unsigned char *d_ws = nullptr, *d_pac = nullptr; char *d_a = nullptr, *d_b = nullptr, *d_oa = nullptr, *d_ob = nullptr; uint32_t *d_off = nullptr;
    const size_t lanes = ((size_t)n + 63) / 64 * 64;
    if (mode != 1) HIPCHK(tmp.alloc((void **)&d_ws, lanes * L.stride));
    HIPCHK(tmp.alloc((void **)&d_a, la + 16)); HIPCHK(tmp.alloc((void **)&d_b, lb + 16));
    HIPCHK(tmp.alloc((void **)&d_oa, tot + 16)); HIPCHK(tmp.alloc((void **)&d_ob, tot + 16)); HIPCHK(tmp.alloc((void **)&d_off, (size_t)(4 * n + 4) * 4));
    uint32_t *d_aoff = d_off, *d_boff = d_off + (n + 1), *d_ooff = d_off + 2 * (n + 1), *d_olen = d_off + 3 * (n + 1);
    HIPCHK(hipMemcpy(d_a, a, la, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_b, b, lb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_aoff, a_off, (size_t)(n + 1) * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_boff, b_off, (size_t)(n + 1) * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_ooff, out_off, (size_t)n * 4, hipMemcpyHostToDevice));
    const unsigned nblk = (unsigned)((n + 63) / 64);
    if (mode == 0) k_probe_nw<<<nblk, 64, 0, c->stream>>>(n, d_aoff, d_boff, d_a, d_b, d_ooff, d_olen, d_oa, d_ob, d_ws, L, c->ix, c->pr);
    else if (mode == 1) k_probe_nw_strips<<<nblk, 64, 0, c->stream>>>(n, d_aoff, d_boff, d_a, d_b, d_ooff, d_olen, d_oa, d_ob, c->ix, c->pr);
    else {
        HIPCHK(tmp.alloc((void **)&d_pac, pac.size()));
        HIPCHK(hipMemcpy(d_pac, pac.data(), pac.size(), hipMemcpyHostToDevice));
        DIndex fx = c->ix;                              // a text that is just the b strings
        fx.pac = d_pac; fx.l_pac = (int64_t)lb; fx.pac_both = 1;
        k_probe_nw_wave<<<nblk, 64, 0, c->stream>>>(n, mode == 3 ? 1 : 0, d_aoff, d_boff, d_a, d_ooff, d_olen, d_oa, d_ob, d_ws, L, fx, c->pr);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out_len, d_olen, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_a, d_oa, tot, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(out_b, d_ob, tot, hipMemcpyDeviceToHost));
    return DG_OK;
}

// RefSequence[g0, g0 + n) as the kernels see it: d_refchar per position (0 outside [0, 2L))
__global__ void __launch_bounds__(256)
k_probe_refseq(const DIndex ix, int64_t g0, int64_t n, char *out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = d_refchar(ix, g0 + i);
}
extern "C" int dg_probe_refseq(dg_ctx *c, int64_t g0, int64_t n, char *out)
{
    if (!c || !out || n < 0 || n > ((int64_t)1 << 30)) return DG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (n == 0) return DG_OK;
    DevTmp tmp;
    char *d_out = nullptr;
    HIPCHK(tmp.alloc((void **)&d_out, (size_t)n));
    k_probe_refseq<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(c->ix, g0, n, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, d_out, (size_t)n, hipMemcpyDeviceToHost));
    return DG_OK;
}

extern "C" int dg_probe_nw(dg_ctx *c, int n, const uint32_t *a_off, const uint32_t *b_off, const char *a, const char *b,
                           uint32_t *out_off, uint32_t *out_len, char *out_a, char *out_b, size_t cap)
{
    return dg_probe_nw_mode(c, 0, n, a_off, b_off, a, b, out_off, out_len, out_a, out_b, cap);
}

// where the dynamic BGZF kernel's time goes: dg_bgzf_compress_flags(DG_BGZF_DYNAMIC) with the kernel's clock sums switched on
extern "C" int dg_probe_bgzf_phases(dg_ctx *c, const void *host_bytes, size_t n, uint64_t cycles[8], size_t *n_bytes, float *device_ms)
{
    if (!c || !host_bytes || !n || !cycles) return DG_ERR_ARG;
    static_assert(BGZF_PHASES == 8, "dartgpu.h says 8");
    c->bam.valid = false; c->bam.bytes = 0; c->bam.ptr = nullptr;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->bam.ready());
    DevTmp tmp;
    unsigned long long *d_ph = nullptr;
    HIPCHK(tmp.alloc((void **)&d_ph, BGZF_PHASES * 8));
    HIPCHK(hipMemsetAsync(d_ph, 0, BGZF_PHASES * 8, c->stream));
    HIPCHK(c->bam.bgzf_in.ensure(n + 8));
    HIPCHK(hipMemcpyAsync(c->bam.bgzf_in.p, host_bytes, n, hipMemcpyHostToDevice, c->stream));
    size_t out_bytes = 0; float ms = 0.f;
    const int rc = bgzf_device(c, c->bam.bgzf_in.p, n, true, &out_bytes, &ms, d_ph);
    if (rc) return rc;
    HIPCHK(hipMemcpy(cycles, d_ph, BGZF_PHASES * 8, hipMemcpyDeviceToHost));
    c->bam.ptr = c->bam.bgzf_out.p; c->bam.bytes = out_bytes; c->bam.valid = true;
    c->bam.ms[0] = 0.f; c->bam.ms[1] = ms;
    if (n_bytes) *n_bytes = out_bytes;
    if (device_ms) *device_ms = ms;
    return DG_OK;
}

// the length builder of the dynamic BGZF coder (dg_bgzf_dyn.h) on a caller's histogram: the one way to its length-limit repair with frequencies a
// strip never has
extern "C" int dg_probe_huff_lengths(dg_ctx *c, const uint32_t *freq, int n_sym, int limit, uint8_t *len_out)
{
    if (!c) return DG_ERR_ARG;
    if (!freq || !len_out || n_sym < 1 || n_sym > (int)BGZF_HUFF_MAX_SYM || limit < 1 || limit > 15) { snprintf(c->err, 512, "dg_probe_huff_lengths: 1 to %u symbols, a limit of 1 to 15", BGZF_HUFF_MAX_SYM); return DG_ERR_ARG; }
    int used = 0;
    for (int i = 0; i < n_sym; i++) {
        if (freq[i] > BGZF_HUFF_FREQ_MAX) { snprintf(c->err, 512, "dg_probe_huff_lengths: frequency %d is above %u", i, BGZF_HUFF_FREQ_MAX); return DG_ERR_ARG; }
        used += freq[i] != 0;
    }
    if (used > (1 << limit)) { snprintf(c->err, 512, "dg_probe_huff_lengths: %d used symbols have no code of at most %d bits", used, limit); return DG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    DevTmp tmp;
    uint32_t *d_freq = nullptr; unsigned char *d_len = nullptr;
    HIPCHK(tmp.alloc((void **)&d_freq, (size_t)n_sym * 4)); HIPCHK(tmp.alloc((void **)&d_len, (size_t)n_sym));
    HIPCHK(hipMemcpy(d_freq, freq, (size_t)n_sym * 4, hipMemcpyHostToDevice));
    k_probe_huff<<<1, BGZF_THREADS, 0, c->stream>>>(d_freq, (uint32_t)n_sym, (uint32_t)limit, d_len);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(len_out, d_len, (size_t)n_sym, hipMemcpyDeviceToHost));
    return DG_OK;
}
