// dart_amd/csrc/api_ctx.h -- what a context owns on the device: buffers, status words, events, and one state struct per library stage.
// Host code of libdartgpu.so, included once by dg_api.hip (one translation unit); not a header for anyone else.

// What a context holds on the device frees itself: every type below releases in its destructor and cannot be copied, so a new member of a stage's state
// struct needs no line in dg_destroy.  dg_destroy makes the context's device current and waits for its stream before `delete c` runs these destructors.
struct NoCopy { NoCopy() = default; NoCopy(const NoCopy &) = delete; NoCopy &operator=(const NoCopy &) = delete; };

template <typename T> struct DBuf : NoCopy {
    T *p = nullptr; size_t cap = 0;
    ~DBuf() { release(); }
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        size_t want = n + n / 8 + 64;
        hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// N status words (or one block of sizes) of a stage on the device and their page-locked copy on the host.  ready() is what every stage calls first: it
// allocates BOTH or NEITHER (d is set last, so a call after a failure starts over, and no caller ever meets d without h) and does nothing the next time.
template <typename T, int N> struct DevStat : NoCopy {
    T *d = nullptr, *h = nullptr;
    ~DevStat() { if (d) (void)hipFree(d); if (h) (void)hipHostFree(h); }
    hipError_t ready(bool zero_device = false) {
        if (d) return hipSuccess;
        T *dd = nullptr, *hh = nullptr;
        hipError_t e = hipMalloc((void **)&dd, N * sizeof(T));
        if (e == hipSuccess && zero_device) e = hipMemset(dd, 0, N * sizeof(T));
        if (e == hipSuccess) e = hipHostMalloc((void **)&hh, N * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) { if (dd) (void)hipFree(dd); return e; }
        memset(hh, 0, N * sizeof(T));
        h = hh; d = dd;
        return hipSuccess;
    }
    hipError_t fetch(hipStream_t s) { return hipMemcpyAsync(h, d, N * sizeof(T), hipMemcpyDeviceToHost, s); }      // all words, device to host
};

// N timing events of a stage: created together (all or none), destroyed together
template <int N> struct EvSet : NoCopy {
    hipEvent_t e[N] = {};
    ~EvSet() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    hipError_t ready() {
        if (e[0]) return hipSuccess;
        hipEvent_t t[N] = {};
        for (int i = 0; i < N; i++) {
            const hipError_t err = hipEventCreate(&t[i]);
            if (err != hipSuccess) { while (i-- > 0) (void)hipEventDestroy(t[i]); return err; }
        }
        for (int i = 0; i < N; i++) e[i] = t[i];
        return hipSuccess;
    }
    hipEvent_t operator[](int i) const { return e[i]; }
    float ms(int i, int j) const { float v = 0.f; (void)hipEventElapsedTime(&v, e[i], e[j]); return v; }
};

// The buffers of one use of the radix sort's pass driver (rs_sort_passes, dg_sort.h): two key and two value buffers, which the stage sizes and fills itself (what they hold
// differs from stage to stage, and so does what the stage says when it cannot have them), and the passes' scratch, which ensure(n) sizes for n pairs.
struct dg_ctx;
struct SortBufs {
    DBuf<uint64_t> k[2]; DBuf<int64_t> v[2]; DBuf<uint32_t> hist, sums;
    const char *short_of = ""; size_t short_bytes = 0;      // after a failed ensure(): the scratch array it could not have, and its size
    hipError_t ensure(uint32_t n);
    int sort(dg_ctx *c, uint32_t n, int bits, int &which);      // n pairs in k / v [which] by the low `bits` bits of the key; which: in = holds the input, out = holds the result
};

// ------------------------------------------------------------------------------------------
// One state struct per library stage, each a member of dg_ctx (dg_api.hip, which holds them by value: they are complete before it): what the stage keeps
// between calls, with its test hooks, reached as c->bi.key.  ready(): the stage's status words and events, allocated on first use.
// ------------------------------------------------------------------------------------------
// SAM text of the batch that ran last (dg_batch_format_sam): per-batch inputs, scan state, the text
struct SamState {
    DBuf<uint32_t> hdr_off, qual_off, qlen; DBuf<char> hdr, qual, text; DBuf<uint64_t> read_off, tile;
    DevStat<unsigned long long, 4> stat;      // total bytes + the three counters
    EvSet<2> ev;
    bool valid = false; size_t bytes = 0;
    size_t first_cap = 0;      // DG_SAM_TEXT_FIRST_CAP: test hook, the first size of the text buffer in bytes (forces the "text outgrew the guess" path)
    hipError_t ready() { const hipError_t e = stat.ready(); return e != hipSuccess ? e : ev.ready(); }
};
// FASTQ text parsed on the device (dg_batch_upload_fastq, dg_fastq.h): the texts, their line starts, the scan state; the batch's names and stored
// qualities stay resident for dg_batch_format_sam_resident in buffers of their own (a dg_batch_format_sam with host arrays uses sam.*).  tail: what the last
// dg_batch_upload_fastq_bgzf left behind the last whole record of each text.
struct FqState {
    DBuf<unsigned char> text, tail; DBuf<uint32_t> lines, tile_cnt, name_at, name_len, loc, hdr_off, qual_off; DBuf<unsigned long long> tile_sum; DBuf<char> hdr, qual;
    DevStat<FqInfo, 1> info;                   // the sizes block
    EvSet<2> ev;
    bool valid = false; size_t hdr_bytes = 0, qual_bytes = 0; float ms = 0.f;      // the batch on the context came from dg_batch_upload_fastq
    bool tail_valid = false; size_t tail_n[2] = {0, 0}, tail_off2 = 0;
    hipError_t ready() { const hipError_t e = info.ready(); return e != hipSuccess ? e : ev.ready(); }
};
// trimming inside the FASTQ upload (dg_set_trim, dg_trim.h): the switches as the kernels take them, a TrimRead per read of the input, the statistics block;
// stats / ms: of the last upload (zeros when it did not trim)
struct TrimState {
    bool on = false; TrimPar par = {};
    bool umi_on = false; dg_umi umi = {};      // dg_set_umi: alone it takes the trimmed path with every step off and min_len 1
    bool any() const { return on || umi_on; }
    TrimPar effective() const {
        TrimPar p = par;
        if (!on) { p = TrimPar{}; p.qual_base = 33; p.min_overlap = 1; p.min_len = 1; }
        if (umi_on) { p.umi_on = 1; p.umi_flags = umi.flags; p.umi_sep = (unsigned char)umi.sep; for (int i = 0; i < 2; i++) { p.umi_len[i] = umi.len[i]; p.umi_skip[i] = umi.skip[i]; } }
        return p;
    }
    DBuf<TrimRead> win;
    DevStat<TrimInfo, 1> info;
    EvSet<2> ev;                               // around the trimming kernels
    uint64_t stats[16] = {}; float ms = 0.f; bool enqueued = false;      // enqueued: the upload under way took the trimmed path
    hipError_t ready() { const hipError_t e = info.ready(); return e != hipSuccess ? e : ev.ready(); }
};
// BGZF inflated on the device (dg_bgzf_inflate, dg_batch_upload_fastq_bgzf; dg_inflate.h): the compressed bytes, the member table, a status word per member,
// the first failing member; out holds the bytes of a dg_bgzf_inflate (the FASTQ path inflates straight into fq.text)
struct InfState {
    DBuf<unsigned char> in, out; DBuf<InfBlock> tab; DBuf<uint32_t> status;
    DevStat<unsigned long long, 1> verdict;
    EvSet<2> ev;
    bool valid = false; size_t bytes = 0;
    hipError_t ready() { const hipError_t e = verdict.ready(); return e != hipSuccess ? e : ev.ready(); }
};
// BAM of the batch that ran last (dg_batch_format_bam, dg_bamfmt.h / dg_bgzf.h): the uncompressed records, the blocks' slots, sizes and places, the
// contiguous stream; bgzf_in holds the bytes of a dg_bgzf_compress.  The records' inputs and scan state are the SAM formatter's buffers (sam.hdr*, sam.qual*,
// sam.qlen, sam.read_off, sam.tile: inputs and scratch of one call); the SAM text itself (sam.text) is left alone.
struct BamState {
    DBuf<unsigned char> rec, bgzf_in, bgzf_slots, bgzf_out; DBuf<uint32_t> bgzf_size; DBuf<uint64_t> bgzf_off;
    DevStat<unsigned long long, 8> stat;      // [0] raw bytes, [1..3] the SAM counters, [4] records, [5] refused, [6] stream bytes
    EvSet<2> ev; float ms[2] = {0.f, 0.f};    // (both phases use the pair, one after the other) / device time of the record kernels, of the BGZF kernels
    bool valid = false; size_t bytes = 0; unsigned char *ptr = nullptr;
    bool rec_valid = false, rec_stored = false; size_t rec_bytes = 0, rec_records = 0;      // rec and the formatter's offsets hold the current batch's records / they are in the store
    size_t first_cap = 0;      // DG_BAM_FIRST_CAP: test hook, the first size of the record buffer in bytes
    hipError_t ready() { const hipError_t e = stat.ready(); return e != hipSuccess ? e : ev.ready(); }
};
// the splice-junction table (dg_sjtab.h): resident across batches; the overflow lists of an insert pass and of the growth behind it; the sorter's buffers,
// the sorted entries and the text of the last dg_sj_finish
struct SjState {
    SjSlot *tab = nullptr; size_t slots = 0, distinct = 0;      // (sj_new_table replaces the table by hand)
    DBuf<dg_sj_entry> ovf[2], in, entries; int ovf_cur = 0;
    SortBufs sort; DBuf<uint64_t> line_off, tile; DBuf<char> text;
    DevStat<unsigned long long, SJ_ST_WORDS> stat;      // SJ_ST_* words
    EvSet<3> ev;                                        // [0], [1]: device time of dg_sj_finish; [2]: the source stream's place for dg_sj_merge
    bool batch_counted = false, fin_valid = false; size_t fin_entries = 0, fin_bytes = 0;
    hipError_t ready() { const hipError_t e = stat.ready(true); return e != hipSuccess ? e : ev.ready(); }
    ~SjState() { if (tab) (void)hipFree(tab); }
};
// the coordinate-sorted BAM store (dg_bamsort.h): resident across batches: the records' bytes, one key and one offset per record, and the list of segments
// (one per accumulate / add call); the sorter's buffers and the sorted array of the last dg_bam_sort_finish
struct BsState {
    unsigned char *rec = nullptr; uint64_t *key = nullptr; int64_t *off = nullptr;      // (bs_grow replaces them by hand, keeping what they hold)
    size_t rec_cap = 0, rec_used = 0, key_cap = 0, off_cap = 0, n = 0, growths = 0;
    std::vector<BsSeg> segs;
    DBuf<uint32_t> cnt_off, tile_cnt; SortBufs sort; DBuf<uint64_t> tile; DBuf<unsigned char> sorted;
    DevStat<unsigned long long, 4> stat;      // [0] bytes of the sorted array, [1] (low word) records counted by k_bs_count
    EvSet<6> ev;                              // [0..4]: the phases of dg_bam_sort_finish; [5]: the source stream's place for dg_bam_sort_merge
    bool fin_valid = false; size_t fin_bytes = 0, fin_records = 0; float ms[4] = {0.f, 0.f, 0.f, 0.f}, acc_ms = 0.f; int passes = 0;
    int fin_which = 0;         // sort.k[fin_which ^ 1] holds the sorted records' places inside their tiles
    size_t first_cap = 0;      // DG_BAMSORT_FIRST_CAP: test hook, the first size of the store in bytes (forces growth)
    hipError_t ready() { const hipError_t e = stat.ready(true); return e != hipSuccess ? e : ev.ready(); }
    ~BsState() { for (void *p : {(void *)rec, (void *)key, (void *)off}) if (p) (void)hipFree(p); }
};
// the BAM index of the sorted array (dg_bamidx.h): the compressed size of every block as the last dg_bam_sort_compress left it (covered: which blocks have one),
// the per-record, per-chunk and per-reference arrays of dg_bam_index_finish, and the index itself
struct BiState {
    DBuf<uint32_t> sizes, sizes_in, span, tile_cnt, chead, mhead, mbin, binq, ref_q, ref_b;
    DBuf<uint64_t> coff, key, voff, excl, ctile, ref_at, lin_at; SortBufs sort;      // sort: the chunks' keys and numbers
    DBuf<unsigned long long> ref, lin; DBuf<unsigned char> flag, out;
    std::vector<unsigned char> covered; std::vector<unsigned long long> h_ref; std::vector<uint64_t> h_lin_at;
    DevStat<unsigned long long, BI_ST_WORDS> stat;      // BI_ST_* words
    EvSet<4> ev;                                        // the kernels before and behind the mid-way wait
    bool valid = false; size_t bytes = 0;
    hipError_t ready() { const hipError_t e = stat.ready(); return e != hipSuccess ? e : ev.ready(); }
};
// the coverage track of the sorted array (dg_coverage.h): buffers of its own (the store's sorter holds the records' places, which the index needs): per record the
// block offsets, per event the sorter's pairs, the scanned deltas and the marks, per breakpoint its key and depth, per entry its breakpoint, record and line
struct CvState {
    DBuf<uint32_t> blk_off, incl, dep_tile, tile_prev, mark, bp_depth, ent_bp, line_off;
    DBuf<uint64_t> blk_tile, tile_last, cnt_tile, bp_key, line_tile, part; SortBufs sort; DBuf<dg_cov_entry> entries; DBuf<char> text;
    DevStat<unsigned long long, CV_ST_WORDS> stat;      // CV_ST_* words
    EvSet<9> ev;                                        // around the kernels between the waits
    bool valid = false; size_t n_entries = 0, bytes = 0; float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f}; int passes = 0;
    hipError_t ready() { const hipError_t e = stat.ready(); return e != hipSuccess ? e : ev.ready(); }
};
// duplicate marking of the sorted array (dg_markdup.h): buffers of its own: per record the end key, the name's hash, the score, the partner and two
// offsets; the sorter's buffers for candidates (then pairs) and for ends; the per-workgroup sums and values
struct MdState {
    DBuf<uint64_t> E, h, tile, junk, part, tile_last;
    SortBufs sort, esort;      // esort: a whole SortBufs on purpose -- a histogram and a sums array of its own (16 words per tile of ends) instead of a pair-only type
    DBuf<uint32_t> score, mate, cand_off, cnt_off, tile_prev;
    DevStat<unsigned long long, MD_ST_WORDS> stat;      // MD_ST_* words
    EvSet<10> ev;
    float ms[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; int passes = 0;
    int hash_bits = MD_HASH_BITS;   // DG_MARKDUP_HASH_BITS: test hook, the bits of a name's hash that are kept (makes collisions and crowded runs reachable)
    hipError_t ready() { const hipError_t e = stat.ready(); return e != hipSuccess ? e : ev.ready(); }
};
// UMI-aware duplicate marking (dg_umidup.h): works in MdState's buffers (the two calls never run at once on a context) and holds what it needs beside them:
// per record U; per item of the list in hand (pairs, then ends) its mark, group, the groups' places, the families' first groups, the winners, the work list
struct UdState {
    DBuf<uint64_t> U, part, tile_h, tile_w;
    DBuf<uint32_t> mark, grp_of, gpos, ffirst, woff, wl; DBuf<unsigned char> win;
    DevStat<unsigned long long, UD_ST_WORDS> stat;      // UD_ST_* words
    EvSet<15> ev;
    float ms[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; int passes = 0;
    hipError_t ready() { const hipError_t e = stat.ready(); return e != hipSuccess ? e : ev.ready(); }
};
// the allele counts of the sorted array (dg_pileup.h): buffers of its own: per record the event offsets, per event the sorter's pairs, the two scanned planes,
// the previous tail and the mark, per distinct allele key its key, sum and depth, per site its first key, its mark and its line's place, per kept site the entry
struct PuState {
    DBuf<uint64_t> ev_off, ev_tile, junk, part, part2, incl_d, incl_a, tile_d, tile_a, tile_last, cnt_tile, ak_key, ak_n, ak_depth, kept_tile, line_tile; SortBufs sort;
    DBuf<uint32_t> tile_prev, prev_tail, mark, site_key, site_mark, line_off; DBuf<dg_site_entry> entries; DBuf<char> text;
    DevStat<unsigned long long, PU_ST_WORDS> stat;      // PU_ST_* words
    EvSet<11> ev;                                       // around the kernels between the waits
    bool valid = false; size_t n_entries = 0, bytes = 0; float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f}; int passes = 0;
    hipError_t ready() { const hipError_t e = stat.ready(); return e != hipSuccess ? e : ev.ready(); }
};
// the QC tables of the sorted array (dg_qc.h): the words, and nothing else: both kernels add into them
struct QcState {
    DBuf<unsigned long long> words;
    EvSet<3> ev;                                        // around the two kernels
    bool valid = false; size_t n_words = 0; float ms[2] = {0.f, 0.f};
    int max_groups = QC_GROUPS;     // DG_QC_MAX_GROUPS: test hook, caps the kernels' grid (a few thousand records drive a workgroup through several trips and flushes)
    hipError_t ready() { return ev.ready(); }
};
// the RNA-seq metrics of the sorted array (dg_rnametrics.h): the words; the per-workgroup lines of both passes; for the depth an event path of its own under
// the stage's filter (per record the block offsets, per event the sorter's pairs and the scanned deltas), so the coverage track's buffers stay what they were
struct RmState {
    DBuf<unsigned long long> words, body; DBuf<uint64_t> line, blk_tile, part; DBuf<uint32_t> blk_off, incl, dep_tile; SortBufs sort;
    DevStat<unsigned long long, CV_ST_WORDS> stat;      // CV_ST_* words: k_cv_count's, and the scanned deltas' total
    EvSet<6> ev;                                        // around the class pass, the counting walk, the event path and the body pass
    bool valid = false; size_t n_words = 0; float ms[3] = {0.f, 0.f, 0.f};
    int max_groups = RM_GROUPS;     // DG_RNA_MAX_GROUPS: test hook, caps the grids of k_rm_class and k_rm_body
    hipError_t ready() { const hipError_t e = stat.ready(); return e != hipSuccess ? e : ev.ready(); }
};
// MD / NM / ts on the sorted array (dg_tags.h): the second array with its records' places and tile sums -- after a call they ARE the store's sorted array
// (dg_bam_tags_finish swaps them with bs.sorted, the sorter's other key buffer and bs.tile), and what lies here is the old one, kept for the next call
struct TgState {
    DBuf<unsigned char> sorted; DBuf<uint64_t> off, tile, junk, part, part2;
    DevStat<unsigned long long, TG_ST_WORDS> stat;      // TG_ST_* words
    EvSet<5> ev;                                        // around the kernels in front of and behind the wait; [4] between the write pass's two
    float ms[2] = {0.f, 0.f}, write_ms[2] = {0.f, 0.f};
    hipError_t ready() { const hipError_t e = stat.ready(); return e != hipSuccess ? e : ev.ready(); }
};
// the gene table (dg_genecount.h): resident across batches, (4 + n_genes) x 3 words, counted under annotation generation gen; the per-workgroup lines of
// the N_* rows; host counts and host records on their way in
struct GcState {
    unsigned long long *counts = nullptr; size_t rows = 0; uint64_t gen = 0; bool nonempty = false, batch_counted = false, timed = false;      // (gc_ready replaces the table by hand)
    DBuf<unsigned long long> wg, in; DBuf<dg_read_out> in_reads; DBuf<dg_report_out> in_rep; DBuf<uint32_t> in_cig;
    EvSet<3> ev;               // [0], [1]: device time of the last count; [2]: the source stream's place for dg_gene_merge
    hipError_t ready() { return ev.ready(); }
    ~GcState() { if (counts) (void)hipFree(counts); }
};
// the class table (dg_txquant.h): resident across batches, CSR, built under annotation generation gen; tab[cur] holds it, a build writes tab[cur ^ 1] and the
// two change places when it has succeeded.  words: the table's eight words; bw: a batch's, added when its classes are in.  Per batch: the units' sizes and
// hashes, the workgroups' lines and sums, the pool (one item per counted unit); per build: the sorter's pairs, the heads, sizes and their sums; a
// downloaded table or host records on their way in; the EM's arrays and the result words of the last dg_tx_finish
struct TxTab { DBuf<uint64_t> off, cnt; DBuf<uint32_t> ids; size_t n_classes = 0, n_members = 0; };
struct TxState {
    TxTab tab[2]; int cur = 0; uint64_t gen = 0; bool made = false, nonempty = false, batch_counted = false, timed = false, fin_valid = false;
    DBuf<unsigned long long> words, bw, wg, tile_sz, tile_items, in_words, S, S2, res;
    DBuf<uint32_t> size, pool_ids, head, sz, sz_ex, scan_sums, in_ids, active, eff, conv; DBuf<uint64_t> hash, pool_off, in_off, in_cnt; DBuf<double> theta;
    DBuf<dg_read_out> in_reads; DBuf<dg_report_out> in_rep; DBuf<uint32_t> in_cig; SortBufs sort;
    DevStat<unsigned long long, 4> pst;       // [0] the pool's ids, [1] its items (k_tx_top); the EM: [0] M, [1] N, [2] workgroups that saw a transcript move
    DevStat<uint32_t, 4> bst;                 // a build: [0] classes, [1] members, [2] a hash collision was seen
    DevStat<unsigned long long, 8> wst;       // the table's words, fetched
    EvSet<7> ev;                              // [0..1] a compatibility pass, [2..3] a part of a build, [4..5] the EM; [6]: the source stream's place for dg_tx_merge
    float ms[3] = {0.f, 0.f, 0.f}; size_t n_words = 0; uint32_t n_tx = 0; unsigned long long strand_mode = 0;      // strand_mode: of the last count (a merge into an empty table brings its own)
    int hash_bits = 64;        // DG_TX_HASH_BITS: test hook, the bits of a list's hash that are kept (forces the collision path); the tables do not depend on it
    hipError_t ready() { hipError_t e = pst.ready(); if (e == hipSuccess) e = bst.ready(); if (e == hipSuccess) e = wst.ready(); return e != hipSuccess ? e : ev.ready(); }
};
