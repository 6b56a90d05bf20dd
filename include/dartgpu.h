/* include/dartgpu.h -- C ABI of libdartgpu.so: DART's per-read mapping path on one MI355X.
 *
 * The drop-in seam is the chunk body of the reference's ReadMapping (Mapping.cpp:598-643):
 * a batch of reads goes in, and for every read the fields that the reference leaves in
 * ReadItem_t (structure.h:149-164: score, sub_score, mis_num, mapq, CanNum, iBestAlnCanIdx,
 * AlnReportArr[]) plus the splice-junction tuples UpdateLocalSJMap (Mapping.cpp:532-565) would
 * have added come out as flat records.  Plain pointers and sizes only; the library owns all
 * device memory; the caller owns the host arrays.  Every entry point returns 0 on success or a
 * negative dg_status; nothing here ever exits the process (the reference's only error
 * behaviour on this path is exit(1) in main.cpp:199-227, which stays in the host program).
 *
 * There is no CPU fallback: without a HIP device dg_init fails with DG_ERR_NO_DEVICE.
 */
#ifndef DARTGPU_H
#define DARTGPU_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dg_ctx dg_ctx;

enum dg_status {
    DG_OK = 0,
    DG_ERR_NO_DEVICE = -1,   /* no HIP device / device index out of range                 */
    DG_ERR_HIP = -2,         /* a HIP call failed; text in dg_last_error                  */
    DG_ERR_ARG = -3,         /* bad argument (NULL, read longer than DG_MAX_RLEN, ...)    */
    DG_ERR_CAPACITY = -4,    /* caller's output arrays too small; `used` holds the need   */
    DG_ERR_INTERNAL = -5,
    DG_ERR_RANGE = -6        /* a field does not fit the compact record types: use the full ones  */
};

#define DG_MAX_RLEN 1000     /* the reference's gz reader caps lines at 1024 bytes (GetData.cpp:186) */

/* The index exactly as the reference loads it (bwt_index.cpp:15-35,102-121,147-159,229-251):
 *   bwt   = contents of PREFIX.bwt after its 40-byte header (Occ-interleaved, 64 B per 128 rows)
 *   sa    = sa[0..n_sa): sa[0] = (uint64)-1, sa[i] = contents of PREFIX.sa after its 56-byte header
 *   pac   = PREFIX.pac, forward strand, 2 bits/base, MSB first
 *   chr_* = per chromosome offset in the forward concatenation and length (PREFIX.ann)        */
typedef struct {
    const uint32_t *bwt; uint64_t bwt_words, primary, L2[5], seq_len;
    const uint64_t *sa;  uint64_t n_sa; int32_t sa_intv;
    const uint8_t  *pac; int64_t l_pac;
    int32_t n_chr; const int64_t *chr_off; const int64_t *chr_len;
} dg_index_view;

/* Globals of the reference that steer the path (main.cpp:101-117,169-192) */
typedef struct {
    int32_t max_gaps;      /* MaxGaps       = 5       */
    int32_t max_dup;       /* MaxDupNum     = 100     (-max_dup, 100..10000)  */
    int32_t max_intron;    /* MaxIntronSize = 500000  (-max_intron)           */
    int32_t min_intron;    /* MinIntronSize = 5       (-min_intron)           */
    int32_t max_mismatch;  /* MaxMismatch   = 0       (-mis)                  */
    int32_t multi_hit;     /* bMultiHit               (-m)                    */
    int32_t all_sj;        /* bFindAllJunction        (-all_sj)               */
    int32_t paired;        /* bPairEnd: reads 2i,2i+1 are mates; mate 2 already
                              reverse-complemented as GetData.cpp:157-162 does */
} dg_params;

/* ReadItem_t after ReadMapping's per-read work (structure.h:149-164) */
typedef struct { int32_t score, sub_score, mis_num, mapq, n_rep, best, rep_off, sj_off, n_sj; } dg_read_out;
/* AlignmentReport_t + Coordinate_t (structure.h:117-141); CIGAR as BAM-style ops len<<4|op,
 * op: M=0 I=1 D=2 N=3 S=4, already merged as GenerateCIGAR does (AlignmentCandidates.cpp:37-61) */
typedef struct { int32_t aln_score, sj_type, flag, paired_idx, chr, bdir; int64_t pos; uint32_t cigar_off, n_cigar; } dg_report_out;
/* one UpdateLocalSJMap key (Mapping.cpp:545-556): forward-strand g1,g2 and the SJ type */
typedef struct { int64_t g1, g2; int32_t type, read_idx; } dg_sj_out;

void        dg_params_default(dg_params *);
/* HIP devices this process can use (0: none, or the runtime failed): a multi-GPU host creates one root context per device and shards its
 * batches over them -- the reference's `-t` threads over one shared index (Mapping.cpp:792-793) */
int         dg_device_count(void);
/* uploads the index to device `device` (0-based HIP ordinal) and builds the device-side layout */
dg_ctx     *dg_init(const dg_index_view *, const dg_params *, int device, int *status);
/* ---- start-up from the index FILES (replaces RestoreReferenceInfo / bwa_idx_load, bwt_index.cpp:147-159,229-253, and main.cpp:231-235) ----
 * The reference reads PREFIX.bwt / .sa / .pac into host arrays and expands RefSequence before the first read is mapped.  Here the
 * three files go from the page cache through page-locked staging chunks straight to HBM (several reader threads, each with its own
 * copy stream; the Occ blocks are re-laid in place chunk by chunk behind their copy), so the host never holds the index.  The host
 * program parses the small text file PREFIX.ann itself (it needs the names for the SAM header) and passes the chromosome table.
 * The look-up aids the kernels build on top of the reference's index -- the full suffix array and the K-mer prefix table, which
 * change no result -- are allocated while the files load and
 *   flags = 0                   built before the call returns (what dg_init does)
 *   flags & DG_INIT_ASYNC_AIDS  allocated and built by a library thread (a quarter of the GPU's wave slots, lowest stream priority) while the
 *                               caller already maps batches: a context picks up each aid at its next batch.
 * dg_index_wait blocks until the aids are complete (DG_OK) or failed (the mapping still works without them; text in dg_last_error).
 * dg_init_report: one line of text with the start-up split in seconds (allocation, file -> HBM, each build kernel); its last two
 * fields, `hw_queues_env_found=<text or unset> hw_queues_env_set=<n>`, are GPU_MAX_HW_QUEUES as the library's load-time constructor
 * found it and as it left it (see dg_clone).                                                                                     */
typedef struct {
    const char *bwt_path, *sa_path, *pac_path;
    int64_t l_pac; int32_t n_chr; const int64_t *chr_off; const int64_t *chr_len;
    uint64_t expected_reads;   /* size of the job if the host knows it (file sizes), 0 = unknown: below 400 M reads the aids are LEAN -- every 4th
                                  SA row, K <= 14: 17 GB instead of 118 GB for a human genome, seeding twice as long -- because the full ones
                                  cost 0.7 s of build kernels and, on memory that was in use a moment ago, seconds of allocation */
} dg_index_files;
#define DG_INIT_ASYNC_AIDS 1
dg_ctx     *dg_init_files(const dg_index_files *, const dg_params *, int device, int flags, int *status);
int         dg_index_wait(dg_ctx *);
const char *dg_init_report(const dg_ctx *);
void        dg_destroy(dg_ctx *);
/* a second context on the same device sharing the parent's index (no copy): its own stream -- one per context -- and batch buffers (keep contexts + 1, the
 * device's copy stream, + the host's own streams <= GPU_MAX_HW_QUEUES: INTEGRATION.md 2.  The library raises that variable to 16 when it
 * loads if it is unset, unparsable or lower, which takes effect in a process that has not initialised HIP yet; dg_clone writes one line
 * to stderr, once per process, when a device's contexts + 2 first exceed the count the library left), so two
 * batches can be in flight at once, one host thread per context -- what the reference gets from running
 * ReadMapping in `-t` threads over one shared index (Mapping.cpp:760-790).  Destroy clones before the parent. */
dg_ctx     *dg_clone(dg_ctx *parent, int *status);
const char *dg_last_error(const dg_ctx *);   /* NULL ctx: error of the last failed dg_init */
int         dg_set_params(dg_ctx *, const dg_params *);

/* ---- the path: host buffers in, host records out (replaces Mapping.cpp:598-639) ----
 * read i = seq[seq_off[i] .. +rlen[i]) ASCII as read from the file.
 * caps/used index: 0 = reports, 1 = cigar ops, 2 = sj tuples.
 * Record layout: reports of read i are reports[rep_off .. rep_off + n_rep) and rep_off increases with i; a report's CIGAR
 * ops are cigar_ops[cigar_off .. cigar_off + n_cigar) -- the layout is the same for the same input (deterministic), but
 * cigar_off does NOT increase with the report index (reports finished by the fused kernel come first, then the others);
 * sj tuples are grouped by read in read order.
 * The whole batch is enqueued on the context's stream without asking the device for a size in between; the call waits twice:
 * for the sizes, then for the records.  If a data-dependent buffer was too small the library grows it and runs the batch
 * again before returning (first batches of a context, or a sudden change in the data).                                   */
int dg_map_batch(dg_ctx *, int n_reads, const uint32_t *seq_off, const uint16_t *rlen, const char *seq,
                 dg_read_out *, dg_report_out *, uint32_t *cigar_ops, dg_sj_out *,
                 const size_t caps[3], size_t used[3]);

/* Page-locked host memory for the arrays handed to dg_map_batch*: with it the copies in and out are DMA transfers that run
 * beside other contexts' kernels; with ordinary memory the calls still work, the runtime stages the copies. */
void *dg_host_alloc(size_t bytes);
void  dg_host_free(void *);

/* The same path for reads that hold nothing but A, C, G, T and N (upper case): 2 bit/base instead of a byte, which matters
 * once the host link is the limit (202 MB -> 56 MB per million 2x101 pairs).
 *   words   read i = words[i * words_per_read ..): 16 bases per word, FIRST base in the TOP two bits (A C G T = 0 1 2 3),
 *           words_per_read = ceil(longest read / 16); an N is stored as any base and listed in nlist
 *   nlist   the N positions as flat base indices  i * 16 * words_per_read + position  (n_n of them, any order)
 *   rlen    per-read lengths, or NULL when every read has length rlen_all
 * A read with any other character (lower case, IUPAC codes, '-') must go through dg_map_batch: the reference compares raw
 * characters in places (tools.cpp:40-47), so such a read maps differently from its upper-case form.                          */
int dg_map_batch_packed(dg_ctx *, int n_reads, int rlen_all, const uint16_t *rlen, int words_per_read, const uint32_t *words,
                        const uint32_t *nlist, size_t n_n, dg_read_out *, dg_report_out *, uint32_t *cigar_ops, dg_sj_out *,
                        const size_t caps[3], size_t used[3]);

/* ---- compact records: the same information in 12 + 16 bytes instead of 36 + 40, and no CIGAR for a plain full-length match ----
 * The host link carries ~57 GB/s per direction on an MI355X box (full duplex for the copy engines: profiles/probes/duplex_probe.hip),
 * so at several hundred million reads per second the bytes of the records load it: 85 -> 30 bytes per read (full records: 545 M
 * reads/s, compact: 860).  Nothing is lost; what the layout already says is not sent:
 *   rep_off    reports lie in read order: a read's reports start at the sum of n_rep of the reads before it
 *   sj_off     likewise the junction tuples: the sum of n_sj of the reads before it
 *   cigar_off  the stored CIGAR ops lie in TWO regions, each in report order: first those of the reports whose `pad` bit 0 is clear (finished
 *              by the fused kernel), behind them those of the reports with the bit set (the general report path); a report's ops start at
 *              the sum of the stored op counts of the reports before it IN ITS REGION (+ the size of the whole first region for the second)
 *   n_cigar    DG_CIGAR_FULL_MATCH (255): the CIGAR is the single op "<length of the report's read>M" and is not stored
 *              (19 of 20 reports of a DNA run); otherwise the number of stored ops (at most 254)
 * Lossless while the fields fit (scores and mismatches < 65536, at most 65535 reports per read / chromosomes, at most 254 CIGAR
 * ops per report, |POS| < 2^31); when one does not, dg_batch_download_compact returns DG_ERR_RANGE and the caller takes the
 * full records with dg_batch_download.  dart_amd/host.py::expand_compact is the reference expansion.                        */
#define DG_CIGAR_FULL_MATCH 255
typedef struct { uint16_t score, sub_score, mis_num; uint8_t mapq, n_sj; uint16_t n_rep, best; } dg_read_c;                             /* 12 bytes */
typedef struct { int32_t pos; uint16_t aln_score, flag; int16_t paired_idx; uint16_t chr /* 0xFFFF = none */;
                 uint8_t n_cigar; int8_t sj_type; uint8_t bdir, pad /* bit 0: stored ops in the second region */; } dg_report_c;            /* 16 bytes */
/* caps[1] counts stored ops (never more than the full records' op count, `used[1]` of dg_batch_run); *n_ops (may be NULL) = how many were written.
 * The compact records are written by the same kernels as the full ones during dg_batch_run / dg_map_batch_compact (not by dg_map_batch /
 * dg_map_batch_packed, whose callers take the full records: DG_ERR_ARG here after those).                                                    */
int dg_batch_download_compact(dg_ctx *, dg_read_c *, dg_report_c *, uint32_t *cigar_ops, dg_sj_out *, const size_t caps[3], size_t *n_ops);
/* upload (ASCII when words == NULL, else packed as dg_map_batch_packed) + run + compact download in one call; used[1] = stored ops */
int dg_map_batch_compact(dg_ctx *, int n_reads, const uint32_t *seq_off, const uint16_t *rlen, const char *seq,
                         int rlen_all, int words_per_read, const uint32_t *words, const uint32_t *nlist, size_t n_n,
                         dg_read_c *, dg_report_c *, uint32_t *cigar_ops, dg_sj_out *, const size_t caps[3], size_t used[3]);

/* ---- the same path split so a caller can keep the batch resident in HBM (bench.py) ----
 * dg_batch_upload copies reads to the device; dg_batch_run runs the whole path on the device
 * leaving the result records in HBM (sizes in `used`); dg_batch_download copies them out.     */
int dg_batch_upload(dg_ctx *, int n_reads, const uint32_t *seq_off, const uint16_t *rlen, const char *seq);
int dg_batch_upload_packed(dg_ctx *, int n_reads, int rlen_all, const uint16_t *rlen, int words_per_read, const uint32_t *words,
                           const uint32_t *nlist, size_t n_n);
int dg_batch_run(dg_ctx *, size_t used[3]);
int dg_batch_download(dg_ctx *, dg_read_out *, dg_report_out *, uint32_t *cigar_ops, dg_sj_out *, const size_t caps[3]);

/* raw device pointers of the last run's records (valid until the next upload/run on this ctx):
 * ptrs[0] dg_read_out[n_reads], [1] dg_report_out[used0], [2] cigar u32[used1], [3] dg_sj_out[used2].
 * Lets a caller hand the records to RCCL (torch.distributed) without a host round trip.       */
int dg_batch_device_ptrs(dg_ctx *, void *ptrs[4]);
/* the compact records of the last dg_batch_download_compact / dg_map_batch_compact in HBM: [0] dg_read_c[n_reads], [1] dg_report_c[used0] */
int dg_batch_device_ptrs_compact(dg_ctx *, void *ptrs[2]);
/* ALL compact records of the last dg_map_batch_compact / dg_batch_download_compact in HBM, with their element counts -- what a multi-GPU
 * host hands to RCCL for the SAM-order gather to the rank that writes (Mapping.cpp:644-664 is ONE ordered writer; bench.py --gather full):
 *   ptrs[0] dg_read_c[counts[0]]   ptrs[1] dg_report_c[counts[1]]   ptrs[2] stored CIGAR ops u32[counts[2]], in the two regions described above
 *   ptrs[3] dg_sj_out[counts[3]], grouped by read in read order (read_idx is the read's index inside the batch)                    */
int dg_batch_device_records_compact(dg_ctx *, void *ptrs[4], size_t counts[4]);

/* ---- SAM text on the device: the last batch's records -> the bytes OutputPairedAlignments / OutputSingledAlignments print (Mapping.cpp:208-369) ----
 * The formatter reads what the batch left in HBM -- the full records and the reads' ASCII bases -- plus the names and qualities given here, and
 * leaves ONE contiguous byte array in HBM: the lines of read 0, read 1, ... in read order, a read's lines in report order.  The bytes are those
 * dart_amd/sam.py::format_records returns for the same records, whatever the launch geometry.
 *   dg_set_chr_names   chromosome i's name = names[name_off[i] .. name_off[i+1]); kept with the index and shared by its clones; n_chr must be
 *                      the index's, else DG_ERR_ARG.  Calling it again replaces the names for every context of the index: it waits for the
 *                      device first, so a text already enqueued keeps the names it started with; a dg_batch_format_sam that is between its
 *                      two launches of the writing kernel at that moment (the rare second launch) returns DG_ERR_ARG instead of mixing names.
 *                      Set the names once, before the batches, as a host program does.
 *   dg_sam_text        read i's name = hdr[hdr_off[i] .. hdr_off[i+1]) (any length), its quality = qual[qual_off[i] .. qual_off[i+1]) in STORED
 *                      order (mate 2's reversed, as its bases are reverse-complemented) and printed as a C string (up to its first NUL byte);
 *                      qual == NULL: FASTA input, the column is '*'.  Reads below n_pair_mode (even, <= n_reads) are mates 2i, 2i+1.
 *   flags              DG_SAM_UNIQUE_ONLY = the reference's -unique; multi-hit output (-m) follows the context's params
 *   counters           [0] unmapped reads, [1] reads with MAPQ 50, [2] reads in shown pairs -- the reference's statistics block
 *   device_ms          device time of the formatter's kernels (may be NULL)
 * dg_batch_format_sam enqueues on the context's stream behind the batch, grows its own device buffers, and waits once, for the size (when
 * the text outgrew the buffer's first guess the writing kernel -- never the batch -- runs a second time).  DG_ERR_ARG, with a text in
 * dg_last_error: no finished batch on the context; no full records (after dg_map_batch_compact); a batch uploaded PACKED (the pipeline keeps
 * no ASCII copy of those reads, so N positions and the bases themselves are not there to print: upload as ASCII); no chromosome names;
 * offsets that decrease; n_pair_mode odd or larger than the batch.  A batch of 0 reads gives 0 bytes.
 * dg_batch_download_sam copies the text out (DG_ERR_CAPACITY, nothing written, when cap < n_bytes); dg_batch_device_sam gives the text in HBM,
 * valid until the next upload or run on this context -- what a multi-GPU host hands to RCCL.
 * dg_last_timings / dg_last_counters keep the batch's values.                                                                              */
typedef struct {
    const uint32_t *hdr_off; const char *hdr;
    const uint32_t *qual_off; const char *qual;
    int32_t n_pair_mode;
} dg_sam_text;
#define DG_SAM_UNIQUE_ONLY 1u
int dg_set_chr_names(dg_ctx *, int n_chr, const uint32_t *name_off, const char *names);
int dg_batch_format_sam(dg_ctx *, const dg_sam_text *in, uint32_t flags, size_t *n_bytes, uint64_t counters[3], float *device_ms);
int dg_batch_download_sam(dg_ctx *, char *out, size_t cap);
int dg_batch_device_sam(dg_ctx *, void **ptr, size_t *n_bytes);

/* ---- FASTQ text on the device: the bytes of the read files -> the batch in HBM (replaces GetNextEntry / GetNextChunk, GetData.cpp:77-179) ----
 * A record is four lines (a line ends with its '\n' or with the text); nothing about '@' or '+' is assumed.  Of a record:
 *   name      IdentifyHeaderBegPos / IdentifyHeaderEndPos (GetData.cpp:55-75) over line 0: behind the leading '@' / '>' characters, up to the first
 *             blank, '/' or tab; empty when the end does not lie behind the begin
 *   read      line 1 without its last byte (GetData.cpp:95-101); a record whose read is empty or missing has no bases: DG_ERR_ARG, the text names it
 *   quality   the first min(read length, length of line 3) bytes of line 3 (GetData.cpp:100-101)
 *   odd reads with rc_odd_reads: kept reverse-complemented through comp_base (everything but ACGTacgt becomes N), the quality reversed
 *             (GetData.cpp:157-166) -- the form dg_params::paired and dg_sam_text expect
 * All other bytes pass through as they are ('\r', lower case, IUPAC codes, '-', NUL).
 *   dg_batch_upload_fastq          texts are any readable host memory (a file mapping works; page-locked memory makes the copy a DMA transfer), each smaller
 *                                  than 2^32 - 256 bytes.  Two texts (GetNextChunk's bSepLibrary, GetData.cpp:141,152): equal record counts, or text1 holds
 *                                  one more, else DG_ERR_ARG.  The copies and six kernels are enqueued on the context's stream; the call waits once, for the
 *                                  sizes.  It leaves the context as dg_batch_upload does (dg_batch_run, the downloads, dg_batch_device_* work unchanged)
 *                                  and the names and stored qualities in HBM beside the bases.  More records than max_reads: DG_ERR_CAPACITY, *n_reads =
 *                                  the need.  A read longer than DG_MAX_RLEN: DG_ERR_ARG.  An error leaves the context usable, without a batch.
 *                                  No text at all: zero reads, DG_OK.
 *   dg_batch_format_sam_resident   dg_batch_format_sam with the names and qualities the FASTQ upload left in HBM (the same launches); DG_ERR_ARG when the
 *                                  context's last upload was not dg_batch_upload_fastq.  dg_batch_format_sam with host arrays still works on such a
 *                                  batch and leaves the resident arrays alone.
 *   dg_batch_download_reads        the parsed batch (GetNextChunk's ReadArr, GetData.cpp:134-179): seq_off / rlen [n_reads], hdr_off / qual_off
 *                                  [n_reads + 1]; caps / used index: 0 = bases, 1 = name bytes, 2 = quality bytes; DG_ERR_CAPACITY: `used` holds the need
 *   dg_batch_fastq_device_ms       device time of the last upload's six kernels (GetData.cpp:77-179 has no counterpart: a measurement)
 *   dg_fastq_tile                  DG_FASTQ_TILE, the bytes of text one workgroup of the line kernels takes (tests place line ends on its seams)       */
#define DG_FASTQ_TILE 16384
typedef struct {
    const char *text1; size_t n1;   /* whole records of file 1 (or of the only file) */
    const char *text2; size_t n2;   /* NULL/0: one file. Else read 2i = record i of text1, 2i+1 = record i of text2 (GetNextChunk's order, GetData.cpp:141,152) */
    int32_t rc_odd_reads;           /* odd reads are stored reverse-complemented, qualities reversed (GetData.cpp:157-166) */
    int32_t max_reads;              /* capacity; more records -> DG_ERR_CAPACITY, *n_reads = the need */
} dg_fastq_text;
int dg_batch_upload_fastq(dg_ctx *, const dg_fastq_text *, int *n_reads);
int dg_batch_format_sam_resident(dg_ctx *, int n_pair_mode, uint32_t flags, size_t *n_bytes, uint64_t counters[3], float *device_ms);
int dg_batch_download_reads(dg_ctx *, uint32_t *seq_off, uint16_t *rlen, char *seq, uint32_t *hdr_off, char *hdr, uint32_t *qual_off, char *qual,
                            const size_t caps[3] /* bases, name bytes, quality bytes */, size_t used[3]);
int dg_batch_fastq_device_ms(dg_ctx *, float *ms);
int dg_fastq_tile(void);

/* ---- BAM on the device: the last batch's records -> uncompressed BAM records -> BGZF blocks, all in HBM (replaces sam_parse1 + sam_write1 of htslib on
 * every SAM line, Mapping.cpp:41-48,655-662,739-755, and the host writer's deflate) ----
 * A record is the bytes the host writer (dart_amd/csrc/host/bam_writer.h, BamWriter::sam_line_to_bam) makes of the SAM line dg_batch_format_sam prints for
 * the same (read, report); the text is never built.  A line the writer refuses -- a name of 0 or more than 254 bytes, a printed quality whose length is not
 * the read's, a CIGAR with an op code of 5 or more (the formatter prints it as '?') -- gives no bytes and is counted.  The blank-joined " XS:A:+" is lost, as in the reference's BAM.  Names hold no tab or newline.
 *   dg_batch_format_bam           inputs, flags and errors as dg_batch_format_sam (no finished batch, compact-only records, a packed upload, no
 *                                 chromosome names, decreasing offsets, a bad n_pair_mode: DG_ERR_ARG with a text; the batch stays usable).  The records lie
 *                                 in read order in one array, the same whatever the launch geometry; the array is then cut into blocks of 0xff00 bytes
 *                                 (the last may be shorter) and every block becomes one BGZF block: gzip / 'BC' header, one raw deflate block (LZ77 with
 *                                 fixed Huffman codes, or stored when that is not smaller), CRC32, ISIZE.  The same input gives the same bytes on every run.
 *                                 *n_bytes <= *n_raw + 31 * blocks.  No BAM header and no end-of-file block: the file's writer adds them (`dart -bo`:
 *                                 BamWriter::open / close).  DG_BAM_RAW: stop at the records.  *n_raw = the records' bytes in both cases.
 *                                 DG_BAM_DYNAMIC: every strip of a block (dg_bgzf_granules [0] input bytes) becomes a deflate block of its own, coded with
 *                                 the smaller of a dynamic Huffman code built from the strip's own tokens and the fixed code (dg_bgzf_dyn.h); the tokens, the
 *                                 stored fallback and the bound on *n_bytes are the same, the stream is smaller.  Ignored together with DG_BAM_RAW.
 *                                 counters [0..2] as dg_batch_format_sam, [3] records written, [4] lines refused.  The call waits twice, for the two sizes;
 *                                 when the records outgrew their buffer's first guess the writing kernel -- never the batch -- runs a second time.
 *                                 A batch of 0 reads gives 0 bytes (0 blocks).  SAM and BAM of one batch may be formatted in either order.
 *   dg_batch_format_bam_resident  the same with the names and qualities dg_batch_upload_fastq left in HBM; DG_ERR_ARG after any other upload
 *   dg_batch_download_bam         copies the result out; DG_ERR_CAPACITY, nothing written, the text names the need, when cap is smaller
 *   dg_batch_device_bam           the result in HBM, valid until the next upload or run on this context
 *   dg_bgzf_compress              any n bytes of host memory -> BGZF blocks on the context's stream (n = 0: no block); needs no batch and no index aids;
 *                                 leaves the result where dg_batch_download_bam / dg_batch_device_bam find it
 *   dg_bgzf_compress_flags        the same with flags: 0 = dg_bgzf_compress, DG_BGZF_DYNAMIC = the coder of DG_BAM_DYNAMIC; any other bit: DG_ERR_ARG, nothing
 *                                 is enqueued and the context stays usable
 *   dg_batch_bam_device_ms        device time of the last call's kernels: [0] the record kernels, [1] the BGZF kernels (0 when that phase did not run)
 *   dg_bgzf_granules              [0] the strip, [1] the segment of the deflate kernel in bytes: matches are looked up in earlier strips (plus distance 1
 *                                 and the same offset of the previous strip) and a lane's match ends with its segment (whole segments at the same distance are then joined, up to 258); tests place repeats on these seams
 * dg_last_timings / dg_last_counters keep the batch's values.                                                                                          */
#define DG_BAM_RAW 2u   /* leave the uncompressed records (no BGZF): what a caller with its own compressor, and the tests, take */
#define DG_BAM_DYNAMIC 4u   /* BGZF with dynamic Huffman codes per strip */
#define DG_BGZF_DYNAMIC 1u  /* the same for dg_bgzf_compress_flags */
int dg_batch_format_bam(dg_ctx *, const dg_sam_text *in, uint32_t flags, size_t *n_bytes, size_t *n_raw,
                        uint64_t counters[5] /* SAM's three, [3] records written, [4] lines refused */, float *device_ms);
int dg_batch_format_bam_resident(dg_ctx *, int n_pair_mode, uint32_t flags, size_t *n_bytes, size_t *n_raw, uint64_t counters[5], float *device_ms);
int dg_batch_download_bam(dg_ctx *, void *out, size_t cap);
int dg_batch_device_bam(dg_ctx *, void **ptr, size_t *n_bytes);
int dg_bgzf_compress(dg_ctx *, const void *host_bytes, size_t n, size_t *n_bytes, float *device_ms);
int dg_bgzf_compress_flags(dg_ctx *, const void *host_bytes, size_t n, uint32_t flags, size_t *n_bytes, float *device_ms);
int dg_batch_bam_device_ms(dg_ctx *, float ms[2]);
int dg_bgzf_granules(int out[2]);

/* ---- BGZF inflated on the device: compressed read files -> a batch in HBM (replaces the gz branch of the reference's reader, GetData.cpp:181-247, for files
 * whose gzip members are BGZF blocks: what bgzip and htslib write, and dg_bgzf_compress) ----
 * A member: magic 1f 8b 08, FLG exactly FEXTRA, a 'BC' subfield (anywhere in the extra field) with the member's size, one raw deflate stream, CRC32 and ISIZE
 * (at most 65536; a member of 0 bytes -- the end-of-file marker -- may stand anywhere).  The call hops over the headers on the host; another FLG, no 'BC'
 * subfield, a size that points past the input, an ISIZE above 65536 or trailing bytes that are no member give DG_ERR_ARG, the text names the block's index,
 * and nothing is enqueued.  One wave inflates one member (dg_inflate.h): RFC 1951 complete, accepting and refusing what zlib's inflate does; then the length
 * against ISIZE and the CRC32.  A block that fails gives DG_ERR_ARG; the text names the block and the first rule it broke.  A malformed block is never read or
 * written outside its own bytes.  A plain single-member gzip file is one serial bit stream: not taken here (FLG / 'BC': DG_ERR_ARG), it stays on the host.
 * Every failure leaves the context usable.
 *   dg_bgzf_inflate               whole blocks in host memory -> their bytes in HBM; needs no batch and no index aids; n = 0: 0 bytes, 0 blocks
 *   dg_inflate_download           copies them out; DG_ERR_CAPACITY, nothing written, when cap is smaller than *n_out was
 *   dg_inflate_device             the bytes in HBM, valid until the next upload, run or inflate on this context
 *   dg_batch_upload_fastq_bgzf    dg_batch_upload_fastq for texts that are pieces of compressed files: text f = head f (plain bytes: the tail the previous
 *                                 call gave back) followed by the bytes of blocks f, each text smaller than 2^32 - 256 bytes.  Blocks do not end where
 *                                 records end, so without `last` only whole records are taken -- four lines, each ended by '\n'; two texts give the same
 *                                 number of records, the smaller of the two counts -- and what lies behind the last record taken is the text's tail:
 *                                 tail[f] (may be NULL) = its size.  With `last` the rules of dg_batch_upload_fastq hold (a line may end with the text,
 *                                 text 1 may hold one more record) and both tails are empty.  Which reads are odd (rc_odd_reads) is counted from the
 *                                 call's first read: pairs interlaced in ONE text need calls that take an even number of records, which this call does
 *                                 not promise.  *n_unlike (may be NULL) counts the records taken that the
 *                                 reference's gz reader (gzgets into 1024 bytes) and its plain reader would read differently: a line of 1024 bytes or
 *                                 more, a NUL in the record, a header line that does not start with '@' or names nothing, a record without bases or
 *                                 with fewer than four lines; the batch is built all the same, the count is what the caller acts on.  Errors as
 *                                 dg_batch_upload_fastq (DG_ERR_CAPACITY: *n_reads = the need), a failing block as above with "text 1" / "text 2".
 *                                 Afterwards the context is as after dg_batch_upload_fastq; dg_batch_fastq_device_ms includes the inflate.  The call
 *                                 waits once.  DG_FQ_CHECK_ONLY: the same verdicts, counts and tails, but no batch is written and the context is left
 *                                 without one (dg_batch_run: DG_ERR_ARG) until the next upload.
 *   dg_batch_download_fastq_tail  the tails of the last dg_batch_upload_fastq_bgzf (the next call's heads); DG_ERR_CAPACITY, nothing written, when a cap
 *                                 is smaller than its tail
 *   dg_inflate_granules           [0] blocks per workgroup, [1] tokens decoded per write-out round of the inflate kernel: tests place seams on them      */
typedef struct {
    const char *head1; size_t n_head1; const void *blocks1; size_t n_blocks1;   /* text 1 = head1 ++ inflate(blocks1) */
    const char *head2; size_t n_head2; const void *blocks2; size_t n_blocks2;   /* blocks2 == NULL && head2 == NULL: one text */
    int32_t rc_odd_reads, max_reads;
    int32_t last;                                                                /* the files end here */
} dg_fastq_bgzf;
#define DG_FQ_CHECK_ONLY 1u   /* inflate, count and check; no batch is written and the context is left without one */
int dg_bgzf_inflate(dg_ctx *, const void *host_bytes, size_t n, size_t *n_out, size_t *n_blocks, float *device_ms);
int dg_inflate_download(dg_ctx *, void *out, size_t cap);
int dg_inflate_device(dg_ctx *, void **ptr, size_t *n_out);
int dg_batch_upload_fastq_bgzf(dg_ctx *, const dg_fastq_bgzf *, uint32_t flags, int *n_reads, size_t tail[2], uint64_t *n_unlike);
int dg_batch_download_fastq_tail(dg_ctx *, char *tail1, size_t cap1, char *tail2, size_t cap2);
int dg_inflate_granules(int out[2]);

/* ---- adapters, poly tails and low-quality ends cut on the device, inside the FASTQ upload (an extension: the reference has no such stage; opt-in per
 * context, unset nothing changes) ----
 * The rules follow cutadapt where that is simple to say (its quality rule, its poly-A rule, its order of steps); this text is the definition, and
 * tests/trim_inputs.py is its sequential twin.  A read is its line 1 as sequenced (L bases s[0..L)) and its quality line cut to the read (ql <= L bytes
 * q[0..ql)), as dg_batch_upload_fastq takes them.  All steps work in file orientation; the reverse complement of a stored mate 2 is applied afterwards to the
 * kept window.  A base compares by its upper case; anything outside ACGT equals nothing.  All arithmetic is integer.
 *   1. quality ends   only when ql == L; else the step is skipped for the read and the read is counted (stats [13]).  v(i) = q[i] - qual_base.
 *                     3' end, qual3 > 0: walk i = L-1 down to 0 with sum += qual3 - v(i); stop at the first sum < 0; b = the i at which sum first reached its
 *                     strict maximum > 0, or L when it never did.  5' end, qual5 > 0: the mirror walk from i = 0; a = i + 1 at the first strict maximum, or 0.
 *                     Both walks see the whole read.  a >= b: the window is empty (a = b = 0; its bases count as cut by the 5' rule up to a, the rest by the 3').
 *   2. adapter        of the read's mate: adapter 0 for reads of text 1, adapter 1 for reads of text 2; in one text, adapter 1 for the odd reads when
 *                     DG_TRIM_PAIRS is set (an interleaved pair text), adapter 0 otherwise.  A length of 0: none.  For p = a .. b - min_overlap ascending:
 *                     n = min(b - p, alen), m = the number of i < n with s[p+i] != A[i]; the first p with m * 1000 <= n * max_err_permille sets b = p.
 *                     Hamming distance only, no indels: a stated limit.
 *   3. poly tails     for each base c in poly_mask the suffix scores S(i) = sum over j = i .. b-1 of (s[j] == c ? +1 : -2), a <= i < b; i* = the smallest i
 *                     with the maximal S; the tail counts when S(i*) > 0 and b - i* >= poly_min; b becomes the smallest counting i* over the enabled bases.
 *   4. length         a read fails when b - a < min_len.  With DG_TRIM_PAIRS reads 2k and 2k+1 are kept or dropped together (a last read without partner
 *                     stands alone).  Kept reads keep their order; the batch is the kept reads, compacted.
 * The stored read is s[a..b), the stored quality q[a..min(b, ql)) (empty when a >= ql), the name unchanged.  Errors of the plain upload keep their meaning on
 * the untrimmed record (a record without bases, a read longer than DG_MAX_RLEN, the count rules of two texts, max_reads against the input count).  A batch of
 * which nothing is left is DG_OK with 0 reads.
 *   dg_set_trim           NULL: off.  Per context, not inherited by dg_clone.  From then on dg_batch_upload_fastq and dg_batch_upload_fastq_bgzf trim (tails,
 *                         n_unlike and DG_FQ_CHECK_ONLY of the latter stay as they are); *n_reads is the kept count; dg_batch_download_reads, the resident
 *                         formatters and every later stage see the trimmed, compacted batch.  The upload still waits once; the trimmed path has kernels of its
 *                         own (dg_trim.h), the plain path keeps its launches.  DG_ERR_ARG with a text, the context usable and its setting as it was: any flag
 *                         bit but DG_TRIM_PAIRS, an adapter longer than 64 bases or with a byte outside ACGT, min_len == 0, min_overlap == 0,
 *                         max_err_permille > 1000, a poly_mask bit above 3, qual3 / qual5 / qual_base above 255.
 *   dg_batch_trim_stats   of the last upload (zeros when it did not trim): [0] reads in, [1] reads kept, [2] bases in, [3] bases kept, [4] bases cut by the 5'
 *                         quality rule, [5] by the 3' quality rule, [6] reads with adapter 0 found, [7] with adapter 1, [8] adapter bases cut, [9] reads with a
 *                         poly tail, [10] poly bases cut, [11] reads that failed the length on their own, [12] reads dropped because the mate failed, [13] reads
 *                         not quality-trimmed because ql < L, [14], [15] zero.  Integer sums: the same whatever the grid.  *device_ms (may be NULL): the
 *                         trimming kernels' device time alone (dg_batch_fastq_device_ms includes them), a measurement.
 *   dg_trim_granules      [0] reads per workgroup of the length kernel, [1] start positions (and walk steps) per round of the cutting kernel: tests place
 *                         drops and read lengths on these seams                                                                                        */
#define DG_TRIM_PAIRS 1u      /* reads 2k and 2k+1 are mates: kept or dropped together; in one text the odd reads take adapter 1 */
typedef struct {
    uint32_t flags;                         /* DG_TRIM_PAIRS */
    uint32_t qual3, qual5, qual_base;       /* 0 = off; base 33 */
    uint32_t min_overlap, max_err_permille; /* 3, 100 */
    uint32_t poly_mask, poly_min;           /* bit 0..3 = A C G T; 10 */
    uint32_t min_len;                       /* >= 1 */
    uint32_t n_adapter[2]; char adapter[2][64];  /* ACGT only */
} dg_trim;
int dg_set_trim(dg_ctx *, const dg_trim *);

/* ---- inline UMIs cut inside the FASTQ upload (dart_amd/csrc/dg_trim.h): what `umi_tools extract` or `fastp --umi` do over the files in front of the mapper.  The
 * first len[m] bases of a read are its UMI, the next skip[m] a linker; both leave the read, and the UMI's letters go to the end of the stored name, where
 * dg_bam_markdup_umi_finish reads them.
 *     slot       of a read: what picks its adapter in dg_set_trim: reads of text 2 take slot 1; the odd reads of one text take slot 1 under DG_UMI_PAIRS; every
 *                other read slot 0
 *     partners   reads 2k and 2k+1 when there are two texts or DG_UMI_PAIRS is set; a last read without a partner stands alone
 *     cut        a read with line 1 = s[0..L) and slot m: u = len[m] + skip[m]; its UMI letters are s[0..len[m]) in upper case, anything outside ACGT as N; the
 *                next skip[m] bases are dropped.  A read with L < u + 1 fails the rule: it and its partner are both dropped -- the rule is pairwise
 *                whatever DG_TRIM_PAIRS says
 *     name       the stored name gains sep, then the read's own letters when it stands alone, else the letters of read 2k followed by those of read 2k+1:
 *                mates keep equal names.  (dg_batch_format_bam's refusal of names above 254 bytes applies to the longer name.)
 *     order      the cut comes first: steps 1-4 of dg_set_trim work on s[u..L) and q[u..ql), "the whole read" meaning that remainder; step 1's condition
 *                compares the untouched ql and L; the stored read is the final window.  dg_set_umi alone takes the trimmed upload path with every step off
 *                and min_len 1; with no UMI set the trimmed path gives the bytes it gave, and the plain path keeps its six launches
 *     stats      dg_batch_trim_stats [14]: the UMI and linker bases removed from reads that passed the rule; [15]: reads dropped by the rule, their own or
 *                their partner's (such a read counts in neither [11] nor [12]).  Both are 0 when the rule is off
 *   dg_set_umi   NULL: off.  Per context, not inherited by dg_clone.  DG_ERR_ARG with a text, the setting left as it was: a flag bit but DG_UMI_PAIRS;
 *                len[0] + len[1] == 0 or > 21; len[m] + skip[m] > DG_MAX_RLEN; sep 0, a blank, a tab, '/' or one of ACGTN+-                          */
#define DG_UMI_PAIRS 1u    /* one text holds pairs: reads 2k, 2k+1 are partners, odd reads take slot 1 */
typedef struct { uint32_t flags; uint32_t len[2], skip[2]; char sep; char pad[3]; } dg_umi;
int dg_set_umi(dg_ctx *, const dg_umi *);
int dg_batch_trim_stats(dg_ctx *, uint64_t stats[16], float *device_ms);
int dg_trim_granules(int out[2]);

/* ---- the splice-junction table on the device: count, sort and print in HBM (replaces UpdateLocalSJMap / UpdateGlobalSJMap, Mapping.cpp:532-577, and
 * OutputSpliceJunctions, Mapping.cpp:683-716) ----
 * Every context owns a table (g1, g2) -> count that stays in HBM across batches: an open-addressing hash table keyed by the full 128 bits, grown by the
 * library.  The same multiset of tuples gives the same entries and the same bytes whatever the order, the batch split, the contexts used or the growth history.
 * Counts are exact up to 2^31 - 1, the reference's int (the table adds in 32 bits).  The one coordinate the table does not hold is INT64_MIN: dg_sj_add
 * refuses such an entry (DG_ERR_ARG, nothing added).  Every failure leaves the context usable; dg_destroy frees the table.
 *   dg_sj_reserve            the table's size in slots, rounded up to a power of two, at least dg_sj_granules [1]; DG_ERR_ARG when the table is not empty
 *   dg_sj_reset              an empty table; the storage is kept
 *   dg_batch_accumulate_sj   counts the tuples sjfinal[0 .. used[2]) of the last finished batch (after full or compact records alike): one launch on the
 *                            context's stream behind the batch, one wait (for the overflow and distinct counts), growth when more than half the slots hold
 *                            a key or a tuple found no slot.  *n_tuples (may be NULL) = used[2].  A batch is counted once: DG_ERR_ARG, with a text in
 *                            dg_last_error, for a second call on the same batch and when the context has no finished batch
 *   dg_sj_add                counts n host entries with their counts (chr is ignored, a count of 0 adds nothing): how a multi-device host folds in the
 *                            table another device downloaded
 *   dg_sj_merge              folds src's table into dst's and leaves src empty; both on one device, ordered behind both contexts' streams; DG_ERR_ARG for
 *                            dst == src or different devices
 *   dg_sj_finish             the entries in ascending signed (g1, g2) order, each with its chromosome (ChrLocMap.lower_bound(g1), Mapping.cpp:683-695), and
 *                            the text "name \t g1+1-off \t g2+1-off \t count \n" of every entry that has one -- the bytes of junctions.tab.  *n_lines = the
 *                            reference's "# of splice junctions".  DG_SJ_ENTRIES_ONLY: no text, *n_bytes = 0; without it the chromosome names must be set
 *                            (DG_ERR_ARG).  The table stays intact: more batches may follow and dg_sj_finish may be called again.  *device_ms (may be NULL):
 *                            device time of the kernels, a measurement.  An empty table: 0 entries, 0 lines, 0 bytes.
 *   dg_sj_download           copies the entries and / or the text of the last dg_sj_finish out (either pointer may be NULL); DG_ERR_CAPACITY, nothing
 *                            written, the text names the need, when a given buffer is too small
 *   dg_sj_device             the same two arrays in HBM, valid until the next table call on the context
 *   dg_sj_granules           [0] the tuples one workgroup of the insert kernel takes, [1] the smallest table in slots                                  */
typedef struct { int64_t g1, g2; uint32_t count; uint32_t chr /* 0xFFFFFFFF: past the last boundary, no line */; } dg_sj_entry;   /* 24 bytes */
#define DG_SJ_ENTRIES_ONLY 1u
int dg_sj_reserve(dg_ctx *, size_t slots);
int dg_sj_reset(dg_ctx *);
int dg_batch_accumulate_sj(dg_ctx *, size_t *n_tuples);
int dg_sj_add(dg_ctx *, const dg_sj_entry *, size_t n);
int dg_sj_merge(dg_ctx *dst, dg_ctx *src);
int dg_sj_finish(dg_ctx *, uint32_t flags, size_t *n_entries, size_t *n_lines, size_t *n_bytes, float *device_ms);
int dg_sj_download(dg_ctx *, dg_sj_entry *entries, size_t cap_entries, char *text, size_t cap_text);
int dg_sj_device(dg_ctx *, void **entries, void **text);
int dg_sj_granules(int out[2]);

/* ---- coordinate-sorted BAM on the device: the records of every batch stay in HBM, one sort at the end (the reference has no such output: an opt-in
 * extension; it replaces the `samtools sort` a user runs behind `dart -bo`) ----
 * Every context owns a store: the bytes of whole uncompressed BAM records, and per record one 64-bit key and its offset.  The order is defined by a record's
 * own bytes -- refID at byte 4, pos at byte 8, flag at byte 18, little endian, read byte by byte (records are not aligned):
 *     tid' = refID when 0 <= refID < n_chr, else n_chr (unplaced records come last)
 *     key  = tid' << 33 | (uint32)(pos + 1) << 1 | (flag >> 4 & 1)
 * ascending key; equal keys keep their input order: ascending ordinal (the caller's number of the batch), then the record's place in its batch; segments with
 * equal ordinals in the order of their calls.  This is the comparison `samtools sort` makes by default (tid as unsigned, pos, reverse strand, stable); no
 * samtools exists where this library is built and tested, so the definition here -- not a run of samtools -- is what the tests pin.
 * The same records under the same ordinals give the same bytes whatever the batch split, the order of the calls, the contexts used or the growth history.
 * Every failure leaves the context and the store usable, with a text in dg_last_error; dg_destroy frees the store.  Memory: the store holds the raw bytes
 * and 16 bytes per record; dg_bam_sort_finish adds the sorted array (the raw bytes again) and 32 bytes per record.  The store grows by doubling and keeps
 * its content (allocate, copy on the context's stream, free); when hipMalloc fails: DG_ERR_CAPACITY, the text names the need, the store stays as it was.
 *   dg_batch_accumulate_bam  appends the uncompressed records the last dg_batch_format_bam[_resident] left for the current batch (with or without
 *                            DG_BAM_RAW): a count pass over the reads (0 to several records each), a scan, an emit pass and a device copy on the context's
 *                            stream, one wait.  DG_ERR_ARG: no records of the current batch are there (no dg_batch_format_bam since the upload / run, or a
 *                            dg_batch_format_sam behind it, which reuses the per-read offsets; dg_bgzf_compress does not count); a second call on the same
 *                            batch.  A batch of 0 records adds nothing.  *n_records / *n_bytes (may be NULL): what was added.
 *   dg_bam_sort_add          whole uncompressed records from host memory: how a multi-device host folds in another device's records.  The host walks them
 *                            once and checks block_size >= 32 + l_read_name + 4 * n_cigar_op + (l_seq + 1) / 2 + l_seq, l_read_name >= 1, refID < n_chr,
 *                            pos >= -1, and that the sizes add up to exactly n; else DG_ERR_ARG, the text names the first bad record, nothing is added.
 *   dg_bam_sort_merge        appends src's store to dst's (its segments behind dst's own) and leaves src empty; both on one device, ordered behind both
 *                            contexts' streams; DG_ERR_ARG for dst == src or different devices
 *   dg_bam_sort_reset        an empty store; the storage is kept
 *   dg_bam_sort_finish       the segments in ordinal order, one stable radix sort over 33 + bits(n_chr) key bits, the records' lengths in sorted order, a
 *                            scan, and a gather into one contiguous array.  The store stays intact: more batches may follow and the call may be repeated.
 *                            An empty store: 0 records, 0 bytes.  The array is valid until the next store call on the context.  *device_ms (may be NULL):
 *                            device time, a measurement; dg_bam_sort_device_ms splits it: [0] segment ordering, [1] the sort (*n_passes passes), [2] lengths
 *                            and scan, [3] the gather, and [4] the key kernels and the copy of the last dg_batch_accumulate_bam.  dg_bam_sort_device: the array in HBM.
 *   dg_bam_sort_compress     one range of the sorted array -> BGZF blocks (flags 0, or DG_BGZF_DYNAMIC), or the bytes as they are (DG_BAM_RAW); the result
 *                            lies where dg_batch_download_bam / dg_batch_device_bam find it.  raw_off must be a multiple of 0xff00 and raw_len such a multiple
 *                            or reach the array's end (else DG_ERR_ARG): so the concatenated output is the same bytes whatever piece size the caller picks,
 *                            and an array of 20 GB never needs 20 GB of block slots at once.  A compressing call also keeps its blocks' compressed sizes
 *                            in HBM for dg_bam_index_finish (4 bytes per block of the array); should that small array not be had, the call succeeds all
 *                            the same and dg_bam_index_finish without block_sizes names the block it misses.
 *   dg_bam_sort_granules     [0] reads per workgroup of the two key kernels, [1] pairs per tile of the sorter, [2] the store's smallest size in bytes    */
int dg_batch_accumulate_bam(dg_ctx *, uint32_t ordinal, size_t *n_records, size_t *n_bytes);
int dg_bam_sort_add(dg_ctx *, const void *records, size_t n, uint32_t ordinal, size_t *n_records);
int dg_bam_sort_merge(dg_ctx *dst, dg_ctx *src);
int dg_bam_sort_reset(dg_ctx *);
int dg_bam_sort_finish(dg_ctx *, size_t *n_records, size_t *n_raw, float *device_ms);
int dg_bam_sort_device_ms(dg_ctx *, float ms[5], int *n_passes);
int dg_bam_sort_device(dg_ctx *, void **ptr, size_t *n_raw);
int dg_bam_sort_compress(dg_ctx *, size_t raw_off, size_t raw_len, uint32_t flags, size_t *n_bytes, float *device_ms);
int dg_bam_sort_granules(int out[3]);

/* ---- the BAM index (.bai) of the sorted array, built in HBM next to the sort (the reference has no such output: an opt-in extension; it replaces the
 * `samtools index` a user runs behind `samtools sort`) ----
 * THE DEFINITION.  The index is the BAI of SAM specification 5.2, built the way htslib's hts_idx_push / hts_idx_finish build it for a BAM read record by
 * record, with two deliberate differences (1, 2 below).  No samtools or htslib binary exists where this library is built and tested: the definition here --
 * not a run of samtools -- is what the tests pin.
 * Per sorted record, fields read byte by byte (block_size at byte 0): refID int32 at byte 4, pos int32 at byte 8, l_read_name u8 at byte 12, n_cigar_op u16 at
 * byte 16, flag u16 at byte 18; the CIGAR ops are u32 little endian (len << 4 | op) from byte 36 + l_read_name.
 *     placed   0 <= refID < n_chr; all other records come last in the sorted array and are only counted, in n_no_coor
 *     mapped   flag & 4 is clear
 *     rlen     the sum of len over ops 0, 2, 3, 7, 8 (M, D, N, =, X) when the record is mapped and n_cigar_op > 0, else 0
 *     end_raw = pos + (rlen ? rlen : 1); beg = max(pos, 0); end = max(end_raw, beg + 1) -- the clamp applies to every placed record (htslib clamps only
 *              mapped ones; the formatter never writes a placed record with pos = -1, so the difference is reachable only through dg_bam_sort_add)
 *     bin      reg2bin(beg, end), recomputed, not read from the record's bin field -- exactly as htslib does
 *     end > 2^29 on a placed record: DG_ERR_RANGE; the text names the record's index and says that such a reference needs a CSI index; no index is left
 *              behind, the sorted array and the store stay as they were
 * Virtual offsets: B = 0xff00; coff[k] = first_block_offset + the compressed sizes of blocks 0 .. k-1; coff[n_blocks] = the file offset behind the last data
 * block.  For a position r of the sorted array voff(r) = coff[r / B] << 16 | r % B for r < n_raw, and voff(n_raw) = coff[n_blocks] << 16: what bgzf_tell returns
 * after reading up to r (a position at a block's end reads as the start of the next block).  Every coff must stay below 2^48, else DG_ERR_RANGE.
 * Chunks, as hts_idx_push makes them: walking the placed records in file order, a chunk is a maximal run of consecutive records with the same (refID, bin),
 * from voff of its first record's start to voff of the start of the record behind the run (behind the last placed record: the first unplaced record's start, or
 * voff(n_raw)).  Per reference the bins are written in ASCENDING BIN NUMBER (difference 1: htslib writes them in hash-table order; the specification allows any
 * order).  Inside a bin the chunks lie in file order; neighbours are merged when prev.end >> 16 >= next.beg >> 16, keeping the earlier begin and the later end
 * (compress_binning's last loop).  htslib's other compression step, moving a bin that spans less than 64 KiB of file to its parent, is NOT done (difference 2:
 * the index is larger and equally valid).
 * The pseudo-bin 37450 is written only for a reference that has records, last: two chunks, (voff of the reference's first record's start, voff of its last
 * record's end) and (n_mapped, n_unmapped).  A reference without records has n_bin = 0 and n_intv = 0.
 * The linear index: n_intv = max over the reference's mapped records of ((end - 1) >> 14) + 1; window w holds the smallest voff(start) over the mapped records
 * with beg >> 14 <= w <= (end - 1) >> 14.  Placed unmapped records are binned and counted but do not touch it.  Empty windows are filled as update_loff fills
 * them: leading ones get the reference's first record's start (the pseudo-bin's first value), a later one its predecessor's value.
 * The bytes, little endian: "BAI\1", int32 n_ref = n_chr; per reference int32 n_bin (counting the pseudo-bin), per bin {u32 bin, int32 n_chunk, n_chunk x
 * {u64 beg, u64 end}}, int32 n_intv, n_intv x u64; finally u64 n_no_coor.  An empty store gives 8 + 8 * n_chr + 8 bytes.
 * The same records and the same block sizes give the same bytes, whatever the grid, the batch split, the contexts used, the store's growth history or the
 * piece size of dg_bam_sort_compress.  The chromosome names are not needed.
 *   dg_bam_index_finish    needs the sorted array of dg_bam_sort_finish with no store call behind it, else DG_ERR_ARG (the text names dg_bam_sort_finish).
 *                          first_block_offset: the file offset of the first block of records (behind the header's blocks).  block_sizes == NULL: the sizes
 *                          dg_bam_sort_compress recorded -- every compressing call (flags 0 or DG_BGZF_DYNAMIC, not DG_BAM_RAW) keeps its blocks' compressed
 *                          sizes in HBM (one u32 per block of the sorted array, copied device to device) and marks the blocks covered; dg_bam_sort_finish and
 *                          every store call clear the marks; a block not compressed since the last finish gives DG_ERR_ARG, the text names the first such
 *                          block.  The sizes are those of the LAST compress of each block: writing those very bytes to the file is the caller's duty.
 *                          block_sizes != NULL (a caller with its own compressor, and the tests): n_blocks must be ceil(n_raw / 0xff00) and every size at
 *                          least 1, else DG_ERR_ARG.  stats (may be NULL): [0] placed records, [1] n_no_coor, [2] bins written, without the pseudo-bins,
 *                          [3] chunks before the merge, [4] chunks after it, [5] linear-index entries.  *device_ms (may be NULL): device time of the
 *                          kernels, a measurement.  The call enqueues on the context's stream and waits twice: for the per-reference sizes, and for the
 *                          index's size.  Memory: 20 bytes per record, about 60 per chunk, 8 per window, and the index; a failed allocation gives
 *                          DG_ERR_CAPACITY, the text names the need.  Every failure leaves the context, the store and the sorted array usable; the
 *                          sorted array stays valid and the call may be repeated, for instance with other sizes.  dg_destroy frees the buffers.
 *   dg_bam_index_download  copies the index out; DG_ERR_CAPACITY, nothing written, when cap is smaller
 *   dg_bam_index_device    the index in HBM, valid until the next store or index call on the context
 *   dg_bam_index_granules  [0] records per workgroup of the per-record kernel, [1] the sorter's tile (chunks)                                              */
int dg_bam_index_finish(dg_ctx *, uint64_t first_block_offset, const uint32_t *block_sizes, size_t n_blocks, size_t *n_bytes, uint64_t stats[6], float *device_ms);
int dg_bam_index_download(dg_ctx *, void *out, size_t cap);
int dg_bam_index_device(dg_ctx *, void **ptr, size_t *n_bytes);
int dg_bam_index_granules(int out[2]);

/* ---- the coverage track of the sorted array, built on the device (dart_amd/csrc/dg_coverage.h): the bedGraph a genome browser shows, as a by-product beside
 * the sort.  The reference has no such output: an opt-in extension (what `bedtools genomecov -bg -split` or `samtools depth` would compute from the file).
 * THE DEFINITION -- modelled on `bedtools genomecov -bg -split` (blocks, 0-based half-open intervals, zero depth not printed) with the default filter of
 * `samtools depth` (FLAG 0x704 skipped); no such tool exists where this library is built and tested, so this text, not a run of one, is what the tests pin.
 * Input: the sorted array of dg_bam_sort_finish with no store call behind it.  The call neither needs nor disturbs dg_bam_sort_compress or
 * dg_bam_index_finish and may come before, between or after them.
 * Per record, fields read byte by byte: refID int32 at byte 4, pos int32 at 8, l_read_name u8 at 12, mapq u8 at 13, n_cigar_op u16 at 16, flag u16 at 18, the
 * CIGAR ops (u32 little endian, len << 4 | op) from byte 36 + l_read_name.  No read ever passes the record's block_size or the array's end.
 *     counted  all of: 0 <= refID < n_chr; pos >= 0; flag & 4 clear; n_cigar_op > 0; (flag & exclude_flags) == 0; mapq >= min_mapq; the strand selection, if
 *              any, passes; the CIGAR lies inside the record (36 + l_read_name + 4 n_cigar_op <= 4 + block_size; dg_bam_sort_add refuses any other record)
 *     strand   s = (flag >> 4 & 1) ^ (flag >> 7 & 1): a second mate counts for the opposite strand.  DG_COV_STRAND_PLUS keeps s == 0, DG_COV_STRAND_MINUS
 *              s == 1; both set, or neither: every record
 *     blocks   walk with p = pos: op 0, 7, 8 (M, =, X) of length L > 0 is a block [p, p + L), then p += L; op 2, 3 (D, N) is p += L and no block; every other
 *              op changes nothing.  Mates that overlap both count.
 *     range    a block end above 2^32 - 1 on a counted record: DG_ERR_RANGE, the text names the record's index; no track is left behind
 *     Positions are not clamped to the chromosome's length (the BAI does not clamp either; the formatter never writes such a record).
 * Depth: every block gives two events, (refID, start, +1) and (refID, end, -1), ordered by refID << 32 | position.  The deltas of equal keys are summed; keys
 * whose sum is 0 are dropped (a read ending where another begins is no breakpoint); the running sum over what remains is the depth from that position to the
 * next.  Every block opens and closes on one reference, so the running sum is 0 at each reference's end.
 * Entries: one dg_cov_entry for every breakpoint with depth > 0, end = the next breakpoint's position; ascending (chr, start); neighbours that touch always
 * differ in depth; a chromosome without coverage has none.  Text: per entry "name\tstart\tend\tdepth\n", decimal, no header line, names of dg_set_chr_names.
 * The result is a function of the record set: the same records give the same bytes whatever their order, the grid, the batch split, the ordinals, the
 * contexts used or the store's growth history.
 *   dg_bam_coverage_finish    flags: DG_COV_ENTRIES_ONLY (no text; the chromosome names are not needed), DG_COV_STRAND_PLUS, DG_COV_STRAND_MINUS; any other
 *                             bit, or no valid sorted array (the text names dg_bam_sort_finish), or text without chromosome names: DG_ERR_ARG.
 *                             exclude_flags: samtools depth's default is 0x704; min_mapq: 0 counts every record.  stats (may be NULL): [0] records counted,
 *                             [1] blocks, [2] breakpoints, [3] entries, [4] covered bases, the sum of end - start, [5] aligned bases, the sum of the blocks'
 *                             lengths (the call checks that it equals the sum of depth x (end - start)), [6] the largest depth.  *device_ms (may be NULL):
 *                             device time of the kernels, a measurement.  More events than the sorter takes (2^32 - 1, less a tile): DG_ERR_CAPACITY, the count in the text.  The call
 *                             enqueues on the context's stream and waits three times: for the number of events, for the numbers of breakpoints and entries,
 *                             and for the text's size.  It uses buffers of its own, never the sorter's (they hold the records' places, which the index
 *                             needs): 4 bytes per record, 40 per event (two per block) and the sorter's histograms, 12 per breakpoint, 24 per entry and its line; a failed
 *                             allocation gives DG_ERR_CAPACITY, the text names the need.  An empty store gives 0 entries and 0 bytes.  Every failure leaves
 *                             the context, the store, the sorted array, the recorded block sizes and a finished index usable; the call may be repeated with
 *                             other filters.  dg_destroy frees the buffers.
 *   dg_bam_coverage_download  copies entries and / or text out (either pointer may be NULL); DG_ERR_CAPACITY, nothing written, when a capacity is too small
 *   dg_bam_coverage_device    entries and text in HBM (NULL when there are none), valid until the next store or coverage call on the context
 *   dg_bam_coverage_device_ms the last finish's device time by stage: [0] the counting walk, [1] the emitting walk, [2] the event sort, [3] the depth and
 *                             breakpoint scans with the compaction, [4] entries and text; *n_passes (may be NULL): the sorter's passes
 *   dg_bam_coverage_granules  [0] records / events / entries per workgroup, [1] the sorter's tile (events)                                                  */
#define DG_COV_ENTRIES_ONLY 1u
#define DG_COV_STRAND_PLUS  2u
#define DG_COV_STRAND_MINUS 4u
typedef struct { uint32_t chr, start, end, depth; } dg_cov_entry;     /* 16 bytes */
int dg_bam_coverage_finish(dg_ctx *, uint32_t flags, uint32_t exclude_flags, uint32_t min_mapq, size_t *n_entries, size_t *n_bytes, uint64_t stats[7], float *device_ms);
int dg_bam_coverage_download(dg_ctx *, dg_cov_entry *entries, size_t cap_entries, char *text, size_t cap_text);
int dg_bam_coverage_device(dg_ctx *, void **entries, void **text);
int dg_bam_coverage_device_ms(dg_ctx *, float ms[5], int *n_passes);
int dg_bam_coverage_granules(int out[2]);

/* ---- duplicate marking of the sorted array, on the device (dart_amd/csrc/dg_markdup.h): flag 0x400 written into the records in HBM, before
 * dg_bam_sort_compress, so that the file, the .bai and the coverage track (default filter 0x704) all see it.  The reference has no such output: an opt-in
 * extension (what `samtools markdup` or Picard MarkDuplicates would compute from the file).
 * THE DEFINITION -- modelled on Picard's rules (unclipped 5' ends, sum of base qualities, a fragment loses to any pair that shares its end); no such tool
 * exists where this library is built and tested, so this text, not a run of one, is what the tests pin (tests/markdup_inputs.py is its sequential twin).
 * Per record, fields read byte by byte, little endian: refID int32 at byte 4, pos int32 at 8, l_read_name u8 at 12, n_cigar_op u16 at 16, flag u16 at 18,
 * l_seq u32 at 20; then from byte 36 the name, the CIGAR ops (u32, len << 4 | op), (l_seq + 1) / 2 bytes of bases and l_seq quality bytes.
 *     examined   all of: 0 <= refID < n_chr; pos >= 0; flag & 4 clear; flag & 0x900 clear; n_cigar_op > 0; name, CIGAR, bases and qualities inside the record
 *                and the array (36 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq <= 4 + block_size).  Every other record plays no part and leaves
 *                with its bytes unchanged.
 *     0x400      the input's bit plays no part: an examined record leaves with the verdict, set or cleared.  The call is idempotent.
 *     end key    s = flag >> 4 & 1; rlen = the sum of M, D, N, =, X; lead / trail = the sum of the S and H ops in front of the first / behind the last op
 *                that is neither (clips alone: lead = their sum, trail = 0); u5 = s ? pos + rlen - 1 + trail : pos - lead in 64-bit arithmetic.
 *                u5 + 2^31 outside [0, 2^33): DG_ERR_RANGE, the text names the record's index in the sorted array, nothing is written.
 *                E = refID << 34 | (u5 + 2^31) << 1 | s
 *     score      the sum of the quality bytes q with 15 <= q <= 93, saturated at 2^20 - 1 (0xff counts as 0)
 *     candidate  an examined record with flag & 1 set, flag & 8 clear, and exactly one of 0x40 and 0x80 set
 *     hash       h = FNV-1a 64 over the l_read_name - 1 name bytes, folded as (h ^ h >> 48), masked to hash_bits bits: 48, or DG_MARKDUP_HASH_BITS = 1..48
 *                from the environment of dg_init (read where DG_BAMSORT_FIRST_CAP is read; a test hook that makes collisions and crowds reachable)
 *     runs       the candidates, ordered stably by h, fall into runs of equal h.  A run of more than 64 is crowded: all its members are fragments.  Else the
 *                candidates of a run with the same name bytes form a group; a group of exactly two, one with 0x40 and one with 0x80, is a pair; members of
 *                any other group are fragments.  A fragment is an examined record that is in no pair.
 *     pairs      lo = min(Ea, Eb), hi = max(Ea, Eb), score = the sum of the members', rep = the smaller of their indices in the sorted array.  Among pairs
 *                with equal (lo, hi) the largest score survives, on equal scores the smallest rep; both records of every other pair get 0x400.
 *     fragments  a fragment with end key E is a duplicate when any pair has lo == E or hi == E, or another fragment with the same E has a larger score, or
 *                an equal score and a smaller index.
 * Optical duplicates and the propagation to secondary or supplementary records are not done; UMIs are dg_bam_markdup_umi_finish's (below).
 *   dg_bam_markdup_finish    works in place on the array of the last dg_bam_sort_finish.  flags: DG_MD_COUNT_ONLY decides and counts but writes no flag; any
 *                             other bit, or no valid sorted array (none finished, or a store call behind the finish; the text names dg_bam_sort_finish):
 *                             DG_ERR_ARG.  stats (may be NULL): [0] examined records, [1] pairs, [2] fragments, [3] duplicate pairs, [4] duplicate fragments,
 *                             [5] candidates in crowded runs, [6] records that leave with 0x400 = 2 [3] + [4], [7] the largest family: pairs sharing one
 *                             (lo, hi).  An empty array gives zeros.  A call that writes also forgets which blocks dg_bam_sort_compress has compressed and
 *                             any finished index or track, exactly as dg_bam_sort_finish does: dg_bam_index_finish without sizes then refuses blocks
 *                             compressed before the marking.  The store itself is untouched: a later dg_bam_sort_finish gives the unmarked array again.
 *                             The call enqueues on the context's stream and waits three times: for the number of candidates (and a record out of range),
 *                             for the numbers of pairs and ends, and for the counts.  Buffers of its own: 32 bytes per record, 32 per candidate (the
 *                             sorter's two key and two value buffers, which the pairs use after the mate search), 32 per end (one per fragment, two per
 *                             pair: at most one per record) and the sorter's histograms; a failed allocation gives DG_ERR_CAPACITY.  Every failure leaves
 *                             the context and the array usable, the array's bytes unchanged.  dg_destroy frees the buffers.
 *   dg_bam_markdup_device_ms  the last finish's device time by stage: [0] the record pass, [1] the mate sort and search, [2] the pair sorts, [3] the end
 *                             sorts, [4] the family scan and the flag writes, [5] counting and emitting pairs and ends; *n_passes (may be NULL): the
 *                             sorter's passes, all sorts together
 *   dg_bam_markdup_granules   [0] records / candidates / pairs / ends per workgroup, [1] the sorter's tile, [2] the largest run that is not crowded        */
#define DG_MD_COUNT_ONLY 1u    /* decide and count, write no flag */
int dg_bam_markdup_finish(dg_ctx *, uint32_t flags, uint64_t stats[8], float *device_ms);
int dg_bam_markdup_device_ms(dg_ctx *, float ms[6], int *n_passes);
int dg_bam_markdup_granules(int out[3]);

/* ---- UMI-aware duplicate marking of the sorted array, on the device (dart_amd/csrc/dg_umidup.h): dg_bam_markdup_finish with the unique molecular identifier
 * at the end of a record's name as one more part of a duplicate's signature.  Highly expressed transcripts put many independent fragments on the same
 * coordinates; marking by position alone flags real molecules as copies.  What `umi_tools dedup` would compute from the finished file, here before
 * dg_bam_sort_compress; no umi_tools exists where this library is built and tested, so this text is what the tests pin (tests/umidup_inputs.py is its twin).
 * THE DEFINITION.  Examined records, end key E, score, candidates, hash, runs, crowded runs, pairs, fragments, DG_ERR_RANGE and the treatment of the input's
 * 0x400 bit are exactly those of dg_bam_markdup_finish.  Beyond them:
 *     U          of an examined record: the name bytes behind the last `sep` of the l_read_name - 1 name bytes.  Valid when 1..21 bytes long and every byte one
 *                of A C G T N + -; those take the codes 1..7, the first letter in the most significant 3-bit field: U = sum of code_i 8^(len - 1 - i), at most 63
 *                bits and never 0.  Every other record has U = 0: no sep, an empty suffix, more than 21 bytes, any other byte (lower case too).  Mates share
 *                their name, so a pair has one U.
 *     pair families   the pairs with equal (lo, hi); a group: those with equal (lo, hi, U); its count: its pairs
 *     end families    every pair gives two ends, (lo, U) and (hi, U), every fragment one, (E, U).  A family: the ends with equal E; a group: those with equal
 *                (E, U), pair ends and fragments alike; its count: its ends
 *     clustering one family's groups each get a root.  max_edit 0: every group is its own root.  A family of more than 64 groups is CROWDED: every group is
 *                its own root (the family is counted for either max_edit).  Else the groups are walked by count descending, then U ascending, and a group g joins
 *                the FIRST earlier group r for which all hold: r is a root; U_r != 0 and U_g != 0; both UMIs have the same length; their letters differ in at most
 *                one place; count_r >= 2 count_g - 1.  Without such an r, g is a root.  One hop only: a group whose only neighbour has itself been absorbed
 *                stays a root (a stated limit against the chains of umi_tools' directional method).
 *     verdicts   among the pairs of a family with equal root the largest score survives, on equal scores the smallest rep; both records of every other such
 *                pair get 0x400.  A fragment is a duplicate when the groups of its end family that share its root hold a pair end, or another fragment with a
 *                larger score, or an equal score and a smaller index.
 * Consequence: when no examined record has a UMI, the bytes and stats[0..7] are those of dg_bam_markdup_finish on the same array, for either max_edit.
 * Limits: Hamming distance 1 only, one hop, 21 letters, and no RX tag is written.
 *   dg_bam_markdup_umi_finish      rules: NULL, max_edit > 1, sep == 0 or any rules->flags bit: DG_ERR_ARG.  flags, the sorted array, the failure texts, what a writing
 *                             call forgets, the three waits and idempotence: as dg_bam_markdup_finish.  stats (may be NULL): [0..6] as there; [7] the largest
 *                             set of pairs sharing one (lo, hi, root); [8] examined records with U != 0; [9] pair families that hold more than one group; [10]
 *                             groups absorbed by another group, pair and end families together; [11] crowded families, both kinds together.  The buffers are
 *                             dg_bam_markdup_finish's and 8 bytes per record, 13 per end and 4 per two ends beside them.
 *   dg_bam_markdup_umi_device_ms   the last finish's device time by stage: [0] the record pass, [1] the mate sort and search, [2] the pair sorts, [3] the end sorts,
 *                             [4] heads, groups and families, [5] the clustering, [6] the flag writes, [7] counting and emitting; *n_passes (may be NULL): the
 *                             sorter's passes (the UMI sorts take only the bits of the largest U, 4 per pass)
 *   dg_bam_markdup_umi_granules    [0..2] as dg_bam_markdup_granules, [3] the largest family that is clustered (64)                                      */
typedef struct { uint32_t flags; uint32_t max_edit /* 0 or 1 */; char sep /* '_' */; char pad[3]; } dg_umi_rules;
int dg_bam_markdup_umi_finish(dg_ctx *, const dg_umi_rules *, uint32_t flags /* DG_MD_COUNT_ONLY */, uint64_t stats[12], float *device_ms);
int dg_bam_markdup_umi_device_ms(dg_ctx *, float ms[8], int *n_passes);
int dg_bam_markdup_umi_granules(int out[4]);

/* ---- allele counts of the sorted array, on the device (dart_amd/csrc/dg_pileup.h): a table of the positions at which a read shows something else than the
 * reference.  The reference program has no such output: an opt-in extension (what `samtools mpileup`, `bam-readcount` or `pysamstats` would compute from the
 * file).  THE DEFINITION -- no pileup tool exists where this library is built and tested, so this text, not a run of one, is what the tests pin
 * (tests/pileup_inputs.py is its sequential twin).
 * Input: the sorted array of dg_bam_sort_finish with no store call behind it.  The call may come before, between or after dg_bam_sort_compress,
 * dg_bam_index_finish and dg_bam_coverage_finish and disturbs none of them; after dg_bam_markdup_finish it sees the marks.
 * Per record, fields read byte by byte as the coverage track reads them, and l_seq, u32 at byte 20, and the bases: base i is the high nibble of byte
 * 36 + l_read_name + 4 n_cigar_op + i / 2 for even i, the low nibble for odd i.
 *     counted  everything the coverage track asks without a strand selection (placed, pos >= 0, mapped, n_cigar_op > 0, (flag & exclude_flags) == 0,
 *              mapq >= min_mapq, the CIGAR inside the record and the array), and: the packed bases inside the record and the array; l_seq > 0; the CIGAR's
 *              read length (the sum of M, I, S, =, X) == l_seq; pos + rlen <= chr_len[refID] (rlen: the sum of M, D, N, =, X).  A record that fails only one
 *              or both of the last two is not counted and tallied in stats[8].
 *     range    a block end above 2^32 - 1 on a record that passes the coverage track's conditions: DG_ERR_RANGE, the text names the record's index, as in the
 *              coverage call.  Tested before the four further conditions: on a chromosome shorter than 2^32 - 1 a block that ends at 2^32 - 1 is a stats[8]
 *              tally, one that ends past it the error.
 *     strand   s = flag >> 4 & 1: the read's orientation, which is what strand-bias filters use -- not the coverage track's transcript strand.
 *     walk     p = pos, q = 0.  M, = or X of length L: read base q + k is observed at reference position p + k for each k < L, then p += L, q += L; a length
 *              above 0 is also a block [p, p + L).  D: every position p .. p + L - 1 gets one DEL observation, p += L.  N: p += L.  I of length L > 0: one INS
 *              observation at the anchor max(p, pos + 1) - 1 (the reference base in front of the insertion, or the read's first position when nothing
 *              precedes it), then q += L.  S: q += L.  H, P: nothing.
 *     alleles  A C G T N DEL INS = 1 .. 7 in the key, 0 .. 6 in the entry.  The reference base at (chr, p) is the base the index's 2-bit text holds at
 *              chr_off[chr] + p, so an N of the FASTA is whatever base the indexer stored.  A read nibble 1, 2, 4, 8 is A, C, G, T; nibble 0 ('=') is the
 *              reference base; every other nibble is N.  A base observation is an event only when its allele differs from the reference base; the CIGAR op
 *              (M, = or X) plays no part in that.
 * Events are ordered by chr << 35 | position << 3 | code with a 64-bit value.  Code 0 is a depth event: every block gives (start, +(1 + (s << 32))) and
 * (end, -(1 + (s << 32))); two 32-bit counters travel in one word.  Codes 1 .. 7 carry 1 + (s << 32).  Depth events sort in front of the allele events of their
 * position, so the running sum of the code-0 values at an allele event is depth | depth_rev << 32 there (starts at the position included, ends excluded); the
 * sum of the values of a run of equal keys is that allele's n | n_rev << 32.
 * Sites: a position with at least one allele event.  n[0..4] count the A, C, G, T and N observed there, the reference allele's own count filled in as depth -
 * (the other four), n_rev likewise: n[0] + .. + n[4] == depth on both strands.  n[5], n[6]: deleted bases and insertions, outside the depth.  top: the
 * non-reference allele, DEL and INS included, with the largest n, ties to the smallest code.  A site is kept when n[top] >= min_alt.  Kept sites ascend in
 * (chr, pos).  The result is a function of the record set: not of order, grid, batch split, ordinals, contexts or growth history.
 * Text: per kept site "name\tpos+1\tR\tdepth\tdepth_rev\tA\tC\tG\tT\tN\tDEL\tINS\tA_rev\t..\tINS_rev\n", decimal, no header line, names of dg_set_chr_names.
 *   dg_bam_pileup_finish      flags: DG_PU_ENTRIES_ONLY (no text; the chromosome names are not needed); any other bit, min_alt == 0, no valid sorted array (the
 *                             text names dg_bam_sort_finish), or text without chromosome names: DG_ERR_ARG.  exclude_flags: 0x704 is the usual filter;
 *                             min_mapq: 0 counts every record.  stats (may be NULL): [0] records counted, [1] blocks, [2] aligned bases, [3] mismatching
 *                             bases, [4] deleted bases, [5] insertions, [6] sites before the min_alt filter, [7] sites kept, [8] records left out for l_seq /
 *                             CIGAR disagreement or for passing their chromosome's end, [9] the largest depth at a kept site.  *device_ms (may be NULL): device
 *                             time of the kernels, a measurement.  More events than the sorter takes (2^32 - 1, less a tile): DG_ERR_CAPACITY, the count in the
 *                             text.  The call enqueues on the context's stream and waits three times: for the number of events, for the numbers of distinct
 *                             allele keys and sites, and for the kept sites and the text's size.  Buffers of its own, never the sorter's or the coverage
 *                             track's: 8 bytes per record, 56 per event and the sorter's histograms, 24 per distinct allele key, 12 per site, 80 per kept site
 *                             and its line; a failed allocation gives DG_ERR_CAPACITY, the text names the need.  An empty store gives 0 sites and 0 bytes.
 *                             Every failure leaves the context, the store, the sorted array, the recorded block sizes, a finished index and a finished track
 *                             usable; the call may be repeated with other filters.  dg_destroy frees the buffers.
 *   dg_bam_pileup_download    copies entries and / or text out (either pointer may be NULL); DG_ERR_CAPACITY, nothing written, when a capacity is too small
 *   dg_bam_pileup_device      entries and text in HBM (NULL when there are none), valid until the next store or pileup call on the context
 *   dg_bam_pileup_device_ms   the last finish's device time by stage: [0] the counting walk, [1] the emitting walk, [2] the event sort, [3] the scans and the
 *                             compaction, [4] sites, entries and text; *n_passes (may be NULL): the sorter's passes
 *   dg_bam_pileup_granules    [0] records / events / sites per workgroup, [1] the sorter's tile (events), [2] reference bases per packed compare step        */
#define DG_PU_ENTRIES_ONLY 1u
typedef struct { uint32_t chr, pos, depth, depth_rev, ref /* 0..3 */, top; uint32_t n[7], n_rev[7]; } dg_site_entry;   /* 80 bytes */
int dg_bam_pileup_finish(dg_ctx *, uint32_t flags, uint32_t exclude_flags, uint32_t min_mapq, uint32_t min_alt, size_t *n_sites, size_t *n_bytes, uint64_t stats[10], float *device_ms);
int dg_bam_pileup_download(dg_ctx *, dg_site_entry *entries, size_t cap_entries, char *text, size_t cap_text);
int dg_bam_pileup_device(dg_ctx *, void **entries, void **text);
int dg_bam_pileup_device_ms(dg_ctx *, float ms[5], int *n_passes);
int dg_bam_pileup_granules(int out[3]);

/* ---- alignment QC of the sorted array, on the device (dart_amd/csrc/dg_qc.h): the flag summary, per-chromosome counts, MAPQ, insert-size and read-length
 * histograms and the per-cycle base / quality / error tables.  The reference program has no such output: an opt-in extension (what `samtools flagstat`,
 * `idxstats` and `stats` and Picard CollectInsertSizeMetrics would compute from the file).  THE DEFINITION -- no samtools exists where this library is built and
 * tested, so this text, not a run of a tool, is what the tests pin (tests/qc_inputs.py is its sequential twin).
 * Input: the sorted array of dg_bam_sort_finish with no store call behind it; read-only on it.  The call may come before, between or after the other stages and
 * disturbs none of them; after dg_bam_markdup_finish it sees the marks.
 * Per record, fields read byte by byte, little endian, as the duplicate marking and the allele counts read them: block_size u32 at byte 0, refID i32 at 4, pos i32
 * at 8, l_read_name u8 at 12, mapq u8 at 13, n_cigar_op u16 at 16, flag u16 at 18, l_seq u32 at 20, next_refID i32 at 24, next_pos i32 at 28, tlen i32 at 32.
 * All counters are u64 words in one flat array, the sections in the order below (dg_bam_qc_offsets gives their first words for a given n_chr).
 *     whole    36 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq <= 4 + block_size, and that size <= the bytes the array holds from the record's start.
 *              A record that is not whole adds 1 to SN.malformed and takes part in nothing else.  primary: flag & 0x900 == 0.  mapped: flag & 4 clear.
 *     FS[2][16]  the flag summary, first index flag >> 9 & 1 (QC fail), every whole record: 0 total, 1 primary, 2 secondary (0x100), 3 supplementary (0x800 without
 *              0x100), 4 duplicates (0x400), 5 primary duplicates, 6 mapped, 7 primary mapped; rows 8 .. 15 count primary records with flag & 1 only: 8 paired,
 *              9 read1 (0x40), 10 read2 (0x80), 11 properly paired (0x2 and mapped), 12 mapped with the mate mapped (0x8 clear), 13 singletons (mapped, 0x8 set),
 *              14 a row-12 record with next_refID != refID, 15 a row-14 record with mapq >= 5.
 *     CH[n_chr + 1][2]  t = refID when 0 <= refID < n_chr, else n_chr: column 0 mapped, column 1 unmapped whole records.
 *     MQ[256]  primary mapped records by mapq.
 *     IS[3][DG_QC_ISIZE]  each pair once: a primary mapped record with flag & 1 set, flag & 8 clear, flag & 0x40 set, next_refID == refID and tlen != 0; bin
 *              min(|tlen|, 8000), |tlen| in 64 bits.  a = flag >> 4 & 1, b = flag >> 5 & 1: a == b is row 2 (other); else f, r = the forward and the reverse
 *              mate's position ((pos, next_pos) when a is 0, (next_pos, pos) when a is 1): f <= r row 0 (inward), f > r row 1 (outward).
 *     RL[2][DG_QC_CYCLES]  primary whole records, mapped or not, by k = flag >> 7 & 1; bin min(l_seq, 511).
 *     profiled a whole record that the allele counts would count (dg_bam_pileup_finish's `counted`) under exclude_flags and min_mapq (0x904 and 0 are the usual
 *              filter); one that passes that filter but is left out there or out of range adds 1 to SN.left_out, and no error is raised for it.
 *     PC[2][12][DG_QC_CYCLES]  every stored base i of a profiled record: class k = flag >> 7 & 1, cycle c = min(s ? l_seq - 1 - i : i, 511), s = flag >> 4 & 1.
 *              Columns 0 .. 4 the base as sequenced, A C G T other: nibbles 1, 2, 4, 8 are A, C, G, T, complemented when s is set; an '=' nibble inside M / = / X is
 *              the reference base, complemented when s is set; everything else ('=' inside I or S too) is other.  5 the quality byte (0xff adds 0); 6 aligned (the
 *              base lies in an M / = / X op); 7 mismatch: aligned, and the allele by the allele counts' rule differs from the reference base at its position;
 *              8 inserted; 9 soft-clipped; 10 insertions: + 1 at the cycle of the first stored base of every I op with len > 0; 11 deletions: + 1 for every D
 *              op with len > 0 at the cycle of stored base max(q, 1) - 1, q the read offset at the op.  Word (k * 12 + column) * 512 + c.
 *     ID[2][DG_QC_INDEL]  profiled records: an I op of length L > 0 in [0][min(L, 64)], a D op in [1][min(L, 64)]; index 0 stays 0.
 *     SN[32]   0 records, 1 malformed, 2 profiled, 3 left_out, 4 bases (the l_seq of primary whole records), 5 profiled bases, 6 aligned, 7 mismatches,
 *              8 inserted bases, 9 deleted bases, 10 clipped, 11 N ops (len > 0), 12 skipped bases, 13 bases without quality (0xff), 14 quality sum, 15 pairs
 *              counted in IS, 16 .. 31 zero.
 * The tables are a function of the record set: not of order, grid, batch split, ordinals, contexts or growth history (integer sums do not depend on order).
 *   dg_bam_qc_finish      flags: none is defined, any bit is DG_ERR_ARG; no valid sorted array: DG_ERR_ARG, the text names dg_bam_sort_finish.  *n_words: the size
 *                         of the array, dg_bam_qc_offsets' [8] for the index's n_chr.  *device_ms (may be NULL): device time of
 *                         the kernels, a measurement.  One wait.  A buffer of its own (the words); a failed allocation gives DG_ERR_CAPACITY.  An empty store
 *                         gives all-zero words.  Every failure leaves the context, the store, the sorted array and every finished stage usable; the call may be
 *                         repeated with another filter.  DG_QC_MAX_GROUPS (read at dg_init) caps the kernels' grid: a test hook, the words do not depend on it.
 *   dg_bam_qc_download    copies the words out; DG_ERR_CAPACITY, nothing written, when cap_words is too small
 *   dg_bam_qc_device      the words in HBM, valid until the next store or QC call on the context
 *   dg_bam_qc_device_ms   the last finish's device time by stage: [0] the per-record tables (lane = record), [1] the per-cycle pass (a quarter wave = record)
 *   dg_bam_qc_granules    [0] threads per workgroup, [1] bases per lane, [2] bases per step of the lanes that share a record, [3] trips between two flushes of the workgroup's table, [4] the
 *                         record length above which per-base terms go straight to the global words
 *   dg_bam_qc_offsets     the first words of FS, CH, MQ, IS, RL, PC, ID, SN for n_chr chromosomes, and [8] the number of words
 *   dg_bam_qc_format      the text of downloaded words, on the host (no context, no device; integers only): "SN\tname\tvalue", "FS\tname\tpassed\tfailed",
 *                         "CH\tname\tlength\tmapped\tunmapped" (the last row `*`, length 0), "MQ\tq\tn", "IS\tsize\tinward\toutward\tother", "RL\tlen\tfirst\tlast",
 *                         "PC\tclass\tcycle+1\tA\tC\tG\tT\tother\tquality\taligned\tmismatch\tinserted\tclipped\tinsertions\tdeletions" (class: first, last),
 *                         "ID\tlen\tins\tdel".  MQ, IS, RL, ID: the rows with a non-zero count; PC: per class the rows up to the last with a non-zero count.  Behind
 *                         the sixteen SN words four derived values, floored, 0 when the denominator is 0: error_ppm = mismatches 10^6 / aligned,
 *                         mean_quality_milli = quality sum 1000 / (profiled bases - bases without quality), insert_mean_milli over the IS bins below 8000,
 *                         insert_median = the smallest size whose cumulative count over all three rows reaches (pairs + 1) / 2; products in 128 bits.
 *                         *n_bytes: the text's size; DG_ERR_CAPACITY, nothing written, when cap is smaller (out may be NULL with cap 0 to ask for the size);
 *                         n_words != the size for n_chr, n_chr < 1 or a missing pointer: DG_ERR_ARG                                                        */
#define DG_QC_CYCLES 512
#define DG_QC_ISIZE 8001
#define DG_QC_INDEL 65
int dg_bam_qc_finish(dg_ctx *, uint32_t flags, uint32_t exclude_flags, uint32_t min_mapq, size_t *n_words, float *device_ms);
int dg_bam_qc_download(dg_ctx *, uint64_t *words, size_t cap_words);
int dg_bam_qc_device(dg_ctx *, void **words);
int dg_bam_qc_device_ms(dg_ctx *, float ms[2]);
int dg_bam_qc_granules(int out[5]);
int dg_bam_qc_offsets(int n_chr, size_t out[9]);
int dg_bam_qc_format(const uint64_t *words, size_t n_words, int n_chr, const char *const *names, const int64_t *lengths, char *out, size_t cap, size_t *n_bytes);

/* ---- MD, NM and ts on the records of the sorted array, on the device (dart_amd/csrc/dg_tags.h): what `samtools calmd` would add to the finished file, written in
 * HBM in front of the first dg_bam_sort_compress.  The reference program has no such output: an opt-in extension.  THE DEFINITION is the comment at the head of
 * dg_tags.h -- no samtools exists where this library is built and tested, so that text, not a run of a tool, is what the tests pin (tests/tags_inputs.py is its
 * sequential twin).  In short: a record the allele counts would count with no filter, whose aux area can be walked, is rewritten: the tags named MD, NM, ts whose
 * flag bit is set are removed, then NM:C/S/I (edit distance: mismatches + inserted + deleted bases, NOT the mapper's mismatch count), MD:Z (as htslib prints it) and
 * ts:A (from the intron motifs GT..AG GC..AG / CT..AC CT..GC of every N op of 4 or more bases; the sign is flipped for a reverse read, minimap2's convention;
 * XS:A is not used because XS:i holds that name) are appended in that order, each when selected; block_size follows.  Every other record is copied verbatim.
 *   dg_bam_tags_finish      needs the sorted array of dg_bam_sort_finish with no store call behind it (else DG_ERR_ARG, the text names dg_bam_sort_finish).
 *                           flags: DG_TAG_MD | DG_TAG_NM | DG_TAG_TS; 0, or any other bit: DG_ERR_ARG, nothing enqueued.  Writes a second array with the same
 *                           records in the same order; afterwards dg_bam_sort_device, dg_bam_sort_compress, dg_bam_markdup_finish, dg_bam_index_finish, the coverage
 *                           track, the allele counts and the QC tables all work on the new array (*n_raw: its size); what they had built over the old bytes
 *                           (compressed sizes, an index, a track, a table) is void, as behind dg_bam_sort_finish.  The store is untouched: another
 *                           dg_bam_sort_finish gives the untagged array again.  A second call with the same flags gives the same bytes as one.  stats (may be NULL):
 *                           [0] records rewritten, [1] copied verbatim: not eligible, [2] copied verbatim: aux area unreadable, [3] old tags removed, [4] mismatches
 *                           and [5] inserted + deleted bases of the rewritten records, [6] ts written, [7] records with an intron and no ts: no motif | conflict
 *                           << 32.  *device_ms (may be NULL): both kernels' device time.  Two waits.  Memory: the new array and 8 bytes per record; the old array's
 *                           buffer is kept for the next call.  A failed allocation: DG_ERR_CAPACITY, the text names the array and its size.  Every failure leaves
 *                           the context, the store and the OLD sorted array valid.  An empty store gives 0 bytes.  The bytes do not depend on the grid, the batch
 *                           split, the contexts or the store's growth history.
 *                           Measured (profiles/tags/tags_rate.json, one MI355X, 2.0 M records of 2x101, 432 MB): 2.42 ms of kernels -- length pass 0.61 ms, write pass
 *                           1.81 ms (2.45 times k_bs_gather's 0.74 ms over the same records) -- beside 17.9 ms of BGZF kernels over the tagged array.
 *   dg_bam_tags_device_ms   the last finish's device time: [0] the length pass (lane = record), [1] the write pass (the new tags, lane = record; the bytes that
 *                           stay, sixteen lanes = record)
 *   dg_bam_tags_granules    [0] records per workgroup of the length pass, [1] lanes per record of the write pass's copy, [2] bases per compare step       */
#define DG_TAG_MD 1u
#define DG_TAG_NM 2u
#define DG_TAG_TS 4u
int dg_bam_tags_finish(dg_ctx *, uint32_t flags, size_t *n_raw, uint64_t stats[8], float *device_ms);
int dg_bam_tags_device_ms(dg_ctx *, float ms[2]);
int dg_bam_tags_granules(int out[3]);

/* ---- gene-level read counts on the device (dart_amd/csrc/dg_genecount.h): a ReadsPerGene table per job ----
 * Counted per batch, from the records the batch left in HBM (mates 2i and 2i + 1 are still neighbours), in a per-context table that stays in HBM across
 * batches and is merged at the end of the job, as the junction table is.  Modelled on `htseq-count --mode union` with the layout of STAR's ReadsPerGene.out.tab;
 * neither tool is run anywhere, so this text is the definition (tests/genecount_inputs.py is its sequential twin):
 * Annotation: n_genes >= 1 genes and n_exons >= 0 exons (chr, start, end, strand, gene): 0 <= chr < n_chr; start < end <= 2^32 - 1, 0-based half-open on the
 *   chromosome; strand 0 (+) or 1 (-); 0 <= gene < n_genes.  Anything else is DG_ERR_ARG, the text names the first bad exon.  Exons may arrive in any order, may
 *   overlap and may repeat.  A gene covers a base on a strand when one of its exons does.  For every base there are three gene sets: `any` (every covering gene),
 *   `plus` (covering genes whose exon strand is +), `minus` (those whose exon strand is -).  Each set gives a label: NONE (0xFFFFFFFF) for the empty set, the
 *   gene's index for exactly one gene, AMBIG (0xFFFFFFFE) for two or more.  The library flattens the annotation once, on the host, into a segment table per
 *   chromosome: ascending breakpoints, per segment the three labels, neighbouring segments with three equal labels merged, the segment behind a chromosome's
 *   last exon NONE.  The table is uploaded once and kept with the index, shared by its clones, as the chromosome names are.  (Gene names are the caller's: the
 *   library prints nothing.)
 * A read's alignment: read k is aligned when reads[k].score > 0 and it has a report j >= best that the SAM formatter would show (aln_score > 0 in pair mode,
 *   aln_score == score otherwise); its alignment is the first such report, the first SAM line the read prints.
 * A read's strand: s = (flag >> 4 & 1) ^ (flag >> 7 & 1) of that report (the coverage track's rule: a second mate counts for the opposite strand).
 * A read's blocks: p = pos - 1 (pos is 1-based); op 0, 7 or 8 of length L > 0 is a block [p, p + L), then p += L; op 2 or 3 moves p and makes no block; every
 *   other op changes nothing.  A read with pos < 1 or chr outside [0, n_chr) has no blocks.
 * A unit: reads 2i, 2i + 1 form one unit for 2i + 1 < n_pair_mode (even, at most n_reads, the meaning it has for dg_batch_format_sam); every read from
 *   n_pair_mode on is a unit of its own.
 * A unit's outcome, decided in this order: 1. no read of the unit is aligned: N_unmapped.  2. an aligned read of the unit has mapq < min_mapq: N_multimapping
 *   (DART's MAPQ takes the values 0, 1, 2, 3 and 50; `dart` passes 4, the -unique rule mapq > 3).  3. otherwise, for each of three columns, the labels of every
 *   segment that every block of every aligned read of the unit touches are combined; a block on a chromosome without segments, or outside them, contributes NONE.
 *   Column 0 (unstranded) reads `any`; column 1 (forward, htseq-count -s yes) reads `plus` when the read's s == 0 and `minus` otherwise; column 2 (reverse) reads
 *   the opposite label; each read uses its own s.  Combine: NONE + x = x, g + g = g, g + h = AMBIG for g != h, AMBIG + x = AMBIG.  Result g: the unit counts
 *   once for gene g in that column (two mates in one gene count once); NONE: N_noFeature of that column; AMBIG: N_ambiguous of that column.  A unit in case 1 or
 *   2 adds to all three columns of its row.
 * Counts: uint64_t counts[4 + n_genes][3]; rows 0-3 are N_unmapped, N_multimapping, N_noFeature, N_ambiguous, row 4 + g is gene g.  Every column sums to the
 *   number of units counted.  The table is a function of the multiset of units: not of their order, the batch split, the grid, the contexts used or the merges.
 * Text (the host's, STAR's layout): "N_unmapped\t%llu\t%llu\t%llu\n" .. "N_ambiguous..", then "name\tc0\tc1\tc2\n" per gene in the caller's gene order.
 * Every failure leaves the context and its table usable, with a text in dg_last_error; dg_destroy frees everything.
 *   dg_gene_set_annotation     flattens, uploads and keeps the table with the index (every clone counts with it); *n_segments (may be NULL): its size.  A second
 *                              call replaces it after waiting for the device, as dg_set_chr_names does.  Each call gives the annotation a new generation number;
 *                              a context's table remembers the generation it was counted under
 *   dg_batch_accumulate_genes  counts the batch that ran last, in one launch sequence on the context's stream behind the batch; *n_units (may be NULL): its
 *                              units.  DG_ERR_ARG with a text: no annotation; no finished batch; no full records (the batch went through dg_map_batch_compact);
 *                              n_pair_mode odd or above the batch; a second call on the same batch; a table that holds counts of an older annotation generation
 *                              (dg_gene_reset first).  A batch of 0 reads adds nothing.  Packed and FASTQ uploads work: no bases are needed
 *   dg_gene_count_records      the same record layout from host memory through the same kernel (a multi-device host; crafted alignments).  The host walks the
 *                              records once: rep_off + n_rep > n_reports, best outside [0, n_rep) on a read with score > 0, or cigar_off + n_cigar > n_ops gives
 *                              DG_ERR_ARG naming the first bad read, and nothing is counted
 *   dg_gene_add                host counts folded in; n_rows must be 4 + n_genes
 *   dg_gene_merge              adds src's table to dst's and leaves src's empty; one device, ordered behind both streams; DG_ERR_ARG for dst == src, different
 *                              devices or different generations
 *   dg_gene_reset              an empty table of the current annotation's shape and generation
 *   dg_gene_download           copies the table out, (4 + n_genes) x 3 words; DG_ERR_CAPACITY, nothing written, when cap_rows is too small (the text names the need)
 *   dg_gene_device             the table in HBM, valid until the next gene call on the context
 *   dg_gene_device_ms          device time of the last accumulate / count_records, a measurement
 *   dg_gene_granules           [0] units per workgroup, [1] the wave width the combining uses                                                        */
typedef struct { int32_t chr; uint32_t start, end, strand, gene; } dg_gene_exon;      /* 20 bytes */
typedef struct { uint32_t n_genes; uint32_t pad; size_t n_exons; const dg_gene_exon *exons; } dg_gene_annot;
int dg_gene_set_annotation(dg_ctx *, const dg_gene_annot *, size_t *n_segments);
int dg_batch_accumulate_genes(dg_ctx *, int n_pair_mode, uint32_t min_mapq, size_t *n_units);
int dg_gene_count_records(dg_ctx *, int n_reads, int n_pair_mode, uint32_t min_mapq, const dg_read_out *reads, const dg_report_out *reports, size_t n_reports,
                          const uint32_t *cigar, size_t n_ops, size_t *n_units);
int dg_gene_add(dg_ctx *, const uint64_t *counts, size_t n_rows);
int dg_gene_merge(dg_ctx *dst, dg_ctx *src);
int dg_gene_reset(dg_ctx *);
int dg_gene_download(dg_ctx *, uint64_t *counts, size_t cap_rows);
int dg_gene_device(dg_ctx *, void **counts);
int dg_gene_device_ms(dg_ctx *, float *ms);
int dg_gene_granules(int out[2]);

/* ---- RNA-seq metrics of the sorted array, on the device (dart_amd/csrc/dg_rnametrics.h): the share of the aligned bases on coding sequence, UTR, introns,
 * intergenic sequence and rRNA, the library's strandedness and the gene-body coverage profile: what Picard CollectRnaSeqMetrics (RSeQC read_distribution.py,
 * infer_experiment.py, geneBody_coverage.py) computes from the finished file.  An opt-in extension, read-only on the sorted array; the reference has no such
 * output.  THE DEFINITION -- no Picard or RSeQC exists where this project is built and tested, so this text is what the tests pin (tests/rnametrics_inputs.py is
 * its sequential twin).
 *   Annotation.  n_tx >= 1 transcripts and their exons, 0-based half-open on the chromosome.  Valid: 0 <= chr < n_chr; strand 0 or 1; no flag bit other than
 *     DG_RNA_TX_RIBOSOMAL; n_exons >= 1 and the exon range inside the exon array; every exon start < end <= 2^32 - 1; cds_start <= cds_end (equal: no CDS).
 *     Anything else is DG_ERR_ARG, the text names the first bad transcript.  Exons of a transcript may come in any order, may overlap and may touch: the library
 *     sorts each transcript's exons and merges those that overlap or touch.  The transcript's span is [first start, last end), its length L the sum of the merged
 *     exons; it is eligible when L >= 100.  Flattened on the host, once, and uploaded; kept with the index and shared by its clones, independent of the gene-count
 *     annotation; a second call replaces the tables after waiting for the device.
 *     class(p) of base p of chromosome c: the maximum over every transcript on c whose span holds p of 4 RIBOSOMAL (p in an exon of a flagged transcript), 3 CODING
 *     (p in an exon and cds_start <= p < cds_end), 2 UTR (p in an exon otherwise; a transcript without CDS is all UTR, as Picard counts it), 1 INTRONIC (p in the
 *     span but in no exon of that transcript); 0 INTERGENIC when no span holds p.  strands(p): the OR of 1 << strand over the transcripts whose span holds p.
 *     The segment table: per chromosome ascending breakpoints, per segment (class, strands), neighbouring segments with equal pairs merged, the segment behind the
 *     last span (0, 0).  *n_segments: its size; *n_eligible: the number of eligible transcripts (either may be NULL).
 *   Records.  A record of the sorted array is counted exactly as the coverage track counts it, under exclude_flags and min_mapq (refID, pos, flag 4 clear,
 *     n_cigar_op > 0, the filter, the CIGAR inside record and array); its blocks are the coverage track's (M, =, X ops with L > 0; D and N move the position).  A
 *     block end above 2^32 - 1 on a counted record: DG_ERR_RANGE, the text names the record's index, no words are left behind.  s = (flag >> 4 & 1) ^ (flag >> 7 & 1).
 *   Words, u64 in one flat array (dg_bam_rna_offsets gives the sections' first words):
 *     BA[5]      every base of every block of every counted record: + 1 at class(p); a block on a chromosome without segments, or outside them, is class 0.
 *     RC[5]      per counted record + 1 at the highest class any of its blocks touches.
 *     ST[4]      per counted record, b = the OR of strands over every segment its blocks touch: b == 0 ST[3] (intergenic); b == 3 ST[2] (ambiguous); otherwise
 *                ST[0] (sense) when s == (b == 2), else ST[1] (antisense).  A second mate already counts for the opposite strand through s.
 *     BC[3][100] the gene-body profile.  depth(c, g): the number of (counted record, block) pairs on c with start <= g < end; it ignores strand.  For an eligible
 *                transcript sample b (0 .. 99) sits at transcript offset o_b = floor((2 b + 1) L / 200); offsets run 5' to 3': over the merged exons from the
 *                left for strand 0, from the right (L - 1 - o_b from the left) for strand 1; mapped through the exons' prefix lengths to a genomic g,
 *                d_b = depth(chr, g).  S = the sum of d_b; the transcript contributes when S >= max(min_cov, 1): BC[0][b] += d_b, BC[1][b] += (d_b > 0),
 *                BC[2][b] += floor(d_b * 100000 / S), its profile in per mille of its own mean (Picard's normalization), in integers.
 *     SN[16]     0 records, 1 counted, 2 blocks, 3 aligned bases (= the sum of BA), 4 transcripts, 5 eligible, 6 contributing, 7 segments, 8 .. 15 zero.
 *   The words are a function of the record set and the annotation: not of order, grid, batch split, ordinals, contexts or growth history.
 *   dg_rna_set_annotation  as above; DG_ERR_ARG leaves the tables of an earlier call in place, and so does a failed allocation or copy of the new tables, which
 *                          gives DG_ERR_HIP with the HIP error's text (as dg_gene_set_annotation does)
 *   dg_bam_rna_finish      flags: none is defined, any bit is DG_ERR_ARG; no valid sorted array: DG_ERR_ARG, the text names dg_bam_sort_finish; no annotation:
 *                          DG_ERR_ARG, the text names dg_rna_set_annotation.  Read-only on the array: it may come before, between or after the other stages and
 *                          disturbs none of them; behind the duplicate marking and the tagging it sees their array.  *n_words: the size of the array
 *                          (dg_bam_rna_offsets' [5]).  *device_ms (may be NULL): device time of the kernels, a measurement.  Buffers of its own; a failed
 *                          allocation gives DG_ERR_CAPACITY.  Every failure leaves the context, the store, the array and every finished stage usable.  Repeatable
 *                          with another filter.  An empty store gives zero BA, RC, ST and BC.  DG_RNA_MAX_GROUPS (read at dg_init) caps the grids: a test
 *                          hook, the words do not depend on it.  A dg_rna_set_annotation of another thread that replaces the tables while the call is being
 *                          prepared or between its two passes: DG_ERR_ARG, the text says so, no words are left; call again.
 *   dg_bam_rna_download    copies the words out; DG_ERR_CAPACITY, nothing written, when cap_words is too small
 *   dg_bam_rna_device      the words in HBM, valid until the next store or RNA-metrics call on the context
 *   dg_bam_rna_device_ms   the last finish's device time by part: [0] the class pass, [1] events, sort and depth, [2] the body pass
 *   dg_bam_rna_granules    [0] records per workgroup trip of the class pass, [1] transcripts per workgroup trip of the body pass
 *   dg_bam_rna_offsets     the first words of BA, RC, ST, BC, SN, and [5] the number of words
 *   dg_bam_rna_format      the text of downloaded words, on the host (no context, no device; integers only, products in 128 bits): "SN\tname\tvalue",
 *                          "BA\tclass\tbases\tppm" (ppm = bases 10^6 / aligned), "RC\tclass\trecords", "ST\tname\trecords", "BC\tbin\tdepth\tcovered\tnormalized".
 *                          Behind the eight SN words four derived ones, floored, 0 when the denominator is 0: sense_ppm = ST[0] 10^6 / (ST[0] + ST[1]),
 *                          five_prime_milli = the sum of BC[2][0 .. 9] / (10 contributing), three_prime_milli the same over bins 90 .. 99, five_to_three_milli =
 *                          1000 x the sum of BC[2][0 .. 9] / the sum of BC[2][90 .. 99].  *n_bytes: the text's size; DG_ERR_CAPACITY, nothing written, when cap is
 *                          smaller (out may be NULL with cap 0 to ask for the size); n_words != the size or a missing pointer: DG_ERR_ARG                     */
#define DG_RNA_TX_RIBOSOMAL 1u
typedef struct { int32_t chr; uint32_t strand /* 0 +, 1 - */, flags /* DG_RNA_TX_RIBOSOMAL */, cds_start, cds_end /* 0-based half-open on the chromosome; equal: no CDS */; uint32_t n_exons; uint64_t first_exon; } dg_rna_tx;      /* 32 bytes */
typedef struct { uint32_t start, end; } dg_rna_exon;   /* 0-based half-open */
typedef struct { uint32_t n_tx; uint32_t pad; size_t n_exons; const dg_rna_tx *tx; const dg_rna_exon *exons; } dg_rna_annot;
int dg_rna_set_annotation(dg_ctx *, const dg_rna_annot *, size_t *n_segments, size_t *n_eligible);
int dg_bam_rna_finish(dg_ctx *, uint32_t flags, uint32_t exclude_flags, uint32_t min_mapq, uint64_t min_cov, size_t *n_words, float *device_ms);
int dg_bam_rna_download(dg_ctx *, uint64_t *words, size_t cap_words);
int dg_bam_rna_device(dg_ctx *, void **words);
int dg_bam_rna_device_ms(dg_ctx *, float ms[3]);
int dg_bam_rna_granules(int out[2]);
int dg_bam_rna_offsets(size_t out[6]);
int dg_bam_rna_format(const uint64_t *words, size_t n_words, char *out, size_t cap, size_t *n_bytes);

/* ---- transcript-level expression on the device (dart_amd/csrc/dg_txquant.h): per batch every unit's set of compatible transcripts, reduced to equivalence
 * classes (ascending transcript list, count) in a class table that stays in HBM across batches; at the end of the job the tables are merged and an EM over the
 * classes gives every transcript its share: what RSEM, or Salmon and kallisto in alignment mode, compute from the finished file.  An opt-in extension; the
 * reference has no such output.  THE DEFINITION -- none of those tools exists where this project is built and tested, so this text is what the tests pin
 * (tests/txquant_inputs.py is its sequential twin).
 *   Annotation.  dg_rna_set_annotation's structs, validity rules and error texts (the first bad transcript is named, a bad call leaves the old tables in
 *     place); cds_* and flags are validated and not used.  Each transcript's exons are sorted, exons that overlap or touch are merged; L_t = the sum of the
 *     merged exons.  The tables (per transcript the merged exons with their prefix lengths; per chromosome a segment table: ascending breakpoints, per segment
 *     the ascending ids of the transcripts with a merged exon over it, neighbouring segments with equal lists merged, the segment behind the last exon empty) are
 *     built on the host once, kept with the index, shared by its clones, independent of the gene-count and RNA-metrics annotations, and carry a generation.
 *   A read's alignment, strand s and blocks: the gene counts' rules, word for word (above).
 *   A read's pieces.  Blocks with L > 0 are joined into one piece across I and D ops (a D's bases belong to the piece); an N op of any length ends a piece, the
 *     next block begins a new one; ops that change nothing change nothing.  A read without blocks has no pieces.
 *   Read r is compatible with transcript t when: it has at least one piece and t is on the read's chromosome; every piece lies wholly inside one merged exon of
 *     t; for consecutive pieces j, j + 1 piece j ends exactly at the end of merged exon e and piece j + 1 starts exactly at the start of merged exon e + 1;
 *     under strand_mode 1 (forward) t's strand == s, under strand_mode 2 (reverse) t's strand != s, strand_mode 0 ignores the strand.
 *   A unit (the gene counts' units), in this order: 1. no read aligned: unmapped; 2. an aligned read has mapq < min_mapq: multimapping; 3. the unit's set is the
 *     intersection of its aligned reads' compatible sets, each read under its own s; empty: incompatible; 4. otherwise counted: + 1 for the class whose list is
 *     the set in ascending id order.
 *   Fragment length, for a counted unit with two aligned reads, on t0 = the set's smallest id: toff(g) = the prefix length of the merged exon that holds g + g -
 *     that exon's start; fl = toff(largest block end - 1) + 1 - toff(smallest block start) over both reads; FL_SUM += fl, FL_N += 1.
 *   Class table, CSR: uint64 off[n_classes + 1], uint32 ids[], uint64 count[], with eight words: units, unmapped, multimapping, incompatible, counted, FL_SUM,
 *     FL_N, 0; units = the sum of the next four.  As a multiset of (list, count) it is a function of the multiset of units: not of their order, the batch split,
 *     the grid, the contexts or the merges.  The order of the classes is not defined.
 *   Effective length.  mean = floor(FL_SUM / FL_N) when FL_N > 0, else frag_mean; eff_t = L_t - mean + 1 when L_t >= mean, else L_t (kallisto's fallback).
 *   EM.  F = 2^20; N = the sum of the counts, N >= 2^33: DG_ERR_RANGE; t is active when a class lists it, M = the number of active transcripts.  M = 0: every
 *     S_t = 0, 0 rounds, converged.  Start: S_t = floor(N F / M) for active t, 0 otherwise.  One round, every floating-point operation one IEEE double operation
 *     without contraction: alpha_t = (double)S_t / F (exact); theta_t = alpha_t / (double)eff_t; per class D = the members' theta added one after the other in
 *     ascending id order from 0.0; D == 0.0: the class gives nothing; otherwise per member q = theta_t / D, x = (double)n_c q, add = (uint64)floor(x 1048576.0),
 *     S'_t += add, an integer sum: S' does not depend on the order of the classes, the grid or the atomics.  conv_r: every t with S'_t >= F has
 *     100 |S'_t - S_t| <= S'_t.  The EM stops after round r when r == max_rounds, or when r is a multiple of 16 and conv_r holds; max_rounds 0 gives the start
 *     values.  `converged` is conv_r of the last round (1 for M = 0; 0 when M > 0 and no round ran).
 *     Result words: S[n_tx], then 16: units, unmapped, multimapping, incompatible, counted, classes, members (the sum of the list lengths), active, rounds,
 *     converged, FL_SUM, FL_N, the mean used, strand_mode (of the context's last count), 0, 0.
 *   dg_tx_set_annotation     as above; *n_exons_merged, *n_segments (either may be NULL): the tables' sizes
 *   dg_batch_accumulate_tx   the units of the batch that ran last, folded into the context's table; *n_units (may be NULL).  DG_ERR_ARG, the table as it was:
 *                            no annotation, no finished batch, a batch counted already, n_pair_mode odd or above the batch, compact records, strand_mode > 2, a
 *                            table of another annotation generation (dg_tx_reset first)
 *   dg_tx_count_records      the same record layout from host memory through the same kernels; the first read whose ranges leave the arrays is named and
 *                            nothing is counted
 *   dg_tx_merge              folds src's table into dst's and leaves src's empty; DG_ERR_ARG for dst == src, two devices or different generations
 *   dg_tx_add                a downloaded table folded in (further roots); lists that are empty or not ascending, ids outside the annotation: DG_ERR_ARG, nothing
 *                            changes, the text names the class
 *   dg_tx_reset              an empty table of the current annotation's generation
 *   dg_tx_classes_size       the table's classes and members
 *   dg_tx_classes_download   off [n_classes + 1], ids, count and the eight words; DG_ERR_CAPACITY, nothing written, the text names the need, when a cap is smaller
 *   dg_tx_finish             the EM over the context's table; flags: none is defined, any bit is DG_ERR_ARG.  Repeatable, leaves the class table as it was.
 *                            *n_words = n_tx + 16; *device_ms (may be NULL): a measurement
 *   dg_tx_download           the result words of the last finish; DG_ERR_CAPACITY, nothing written, when cap_words is too small
 *   dg_tx_device             the same words in HBM, valid until the next dg_tx_* call on the context
 *   dg_tx_device_ms          device time by part: [0] the compatibility passes and [1] the class building of the last count, merge or add, [2] the last EM
 *   dg_tx_granules           [0] units per workgroup of the compatibility passes, [1] the wave width
 *   dg_tx_word_name          the name of summary word i (0 .. 15) as dg_tx_format prints it; NULL for any other i
 *   dg_tx_format             the text of downloaded result words, on the host (no context, no device; integers only, products in 128 bits): "# name\tvalue"
 *                            per summary word, "transcript_id\tlength\teff_length\test_counts\ttpm", then one line per transcript in the caller's order:
 *                            est_counts = floor(S_t 1000 / F) printed as %llu.%03llu; rate_t = floor(S_t 1024 / eff_t), R = the sum of the rates; tpm in
 *                            thousandths = floor(rate_t 10^9 / R), 0 when R = 0, printed the same way.  a: the annotation the words were made under (for L_t);
 *                            names: n_tx strings.  *n_bytes: the text's size; DG_ERR_CAPACITY, nothing written, when cap is smaller (out may be NULL with cap 0)
 * Every failure leaves the context, the batch, the table and the other stages usable.  DG_TX_HASH_BITS (read at dg_init) truncates the lists' hashes: a test
 * hook that forces the path for colliding hashes, the tables do not depend on it.                                                                       */
int dg_tx_set_annotation(dg_ctx *, const dg_rna_annot *, size_t *n_exons_merged, size_t *n_segments);
int dg_batch_accumulate_tx(dg_ctx *, int n_pair_mode, uint32_t min_mapq, uint32_t strand_mode, size_t *n_units);
int dg_tx_count_records(dg_ctx *, int n_reads, int n_pair_mode, uint32_t min_mapq, uint32_t strand_mode, const dg_read_out *reads, const dg_report_out *reports, size_t n_reports,
                        const uint32_t *cigar, size_t n_ops, size_t *n_units);
int dg_tx_merge(dg_ctx *dst, dg_ctx *src);
int dg_tx_add(dg_ctx *, const uint64_t *off, const uint32_t *ids, const uint64_t *count, size_t n_classes, const uint64_t *words8);
int dg_tx_reset(dg_ctx *);
int dg_tx_classes_size(dg_ctx *, size_t *n_classes, size_t *n_members);
int dg_tx_classes_download(dg_ctx *, uint64_t *off, uint32_t *ids, uint64_t *count, size_t cap_classes, size_t cap_members, uint64_t *words8);
int dg_tx_finish(dg_ctx *, uint32_t flags, uint64_t frag_mean, uint32_t max_rounds, size_t *n_words, float *device_ms);
int dg_tx_download(dg_ctx *, uint64_t *words, size_t cap_words);
int dg_tx_device(dg_ctx *, void **words, size_t *n_words);
int dg_tx_device_ms(dg_ctx *, float ms[3]);
int dg_tx_granules(int out[2]);
const char *dg_tx_word_name(int i);
int dg_tx_format(const uint64_t *words, size_t n_words, const dg_rna_annot *a, const char *const *names, char *out, size_t cap, size_t *n_bytes);

/* per-kernel device time of the last dg_batch_run, measured with HIP events on the library's
 * stream: names[i] -> ms[i]; returns the number of entries written (<= cap)                   */
int dg_last_timings(dg_ctx *, const char **names, float *ms, int cap);
/* work counters of the last run: [0] Occ-pair steps [1] Occ blocks touched [2] LF steps
 * [3] SA lookups [4] seeds [5] candidates [6] NW calls [7] NW cells [8] reseed calls
 * [9] reseed window bases -- [0..3] are counted as the REFERENCE's algorithm would execute them
 * (the basis of the algorithmic-byte figure); [10] Occ-pair steps and [11] Occ blocks this
 * implementation really executed, [12] k-mer prefix-table look-ups, [13] LF steps really executed, [14..17] seeding statistics,
 * [18] 512-position trips of k_reseed's waves, [19] the time its waves were resident, summed, in 10 ns ticks,
 * [20..24] wave-trips of the seeding kernel per queue (begin, Occ step, text comparison, locate, refill), [25..29] the slots they served,
 * [30] its phases, summed over the workgroups (a phase can serve four wave-trips),
 * [31..35] the time the waves of k_seed_qf, k_seed_heavy, k_chain_heavy, k_pair, k_report were resident, summed over the waves, in 10 ns ticks,
 * [36] units (pairs / single reads) that took the general report path, [37] units chained by a wave each (> 16 seeds),
 * [38] how many times the batch was enqueued (> 1: a capacity estimate was too small and the batch ran again),
 * [39] / [40] how often this context has run a batch again since it was created: capacity grown / a scan that did not complete   */
int dg_last_counters(dg_ctx *, uint64_t *out, int cap);

/* diagnostic (tests/probes/kpair_wait.py): the per-tile trace of one of the last run's single-pass scans -- 4 u64 per tile: epoch << 32 | HW_ID,
 * wall clock at the ticket, at the publication of the tile's own totals, XCC_ID << 56 | wall clock at the publication of its prefix.
 * which: 0 = seed offsets, 1 = the fused pair kernel, 2 = the general path's emit kernel.  DG_ERR_CAPACITY: *n_tiles holds the need. */
int dg_debug_scan_trace(dg_ctx *, int which, uint64_t *out, size_t cap_tiles, size_t *n_tiles, double *ticks_per_ms);

/* ---- the index builder's sorter (replaces the suffix sorting inside BWT_Index/bwtindex.c:77-148) ----
 * Stable radix sort of n < 2^32 (key, value) pairs in DEVICE memory, ascending by the low key_bits bits of the key; keys/vals hold the
 * input and the result, *_tmp are scratch of the same size.  Runs on the device's NULL stream and returns when done.
 * dart_amd/index_build.py drives it (prefix doubling: one sort of (rank pair, suffix) per round).                              */
int dg_sort_pairs(int device, uint64_t *keys, int64_t *vals, uint64_t *keys_tmp, int64_t *vals_tmp, size_t n, int key_bits);
/* The same passes alone, timed: the histograms are allocated before the first event and freed after the second, and nothing is copied back, so the sorted
 * pairs may end in keys_tmp / vals_tmp (*in_tmp = 1).  *ms: the device time of the passes.  A yardstick for profiles/probes, n >= 2.               */
int dg_probe_sort_passes(int device, uint64_t *keys, int64_t *vals, uint64_t *keys_tmp, int64_t *vals_tmp, size_t n, int key_bits, float *ms, int *in_tmp);

/* ---- stage probes (parity tests of single kernels; mirror oracle/dart_oracle.h) ----
 * seeds of every read after the (gPos,rPos) sort (IdentifySeedPairs, AlignmentCandidates.cpp:181-215):
 * read i owns [seed_off[i], seed_off[i+1]) of rpos/slen/gpos; seed_off has n_reads+1 entries. */
int dg_probe_seeds(dg_ctx *, int n_reads, const uint32_t *seq_off, const uint16_t *rlen, const char *seq,
                   uint32_t *seed_off, int32_t *rpos, int32_t *slen, int64_t *gpos, size_t cap, size_t *used);
/* nw_alignment (nw_alignment.cpp:18-82) of n pairs: a[i]=s[a_off[i]..a_off[i+1]) etc.; outputs are
 * NUL-free gapped strings of equal length out_len[i] at out_a/out_b + out_off[i] (cap each = sum of lengths) */
int dg_probe_nw(dg_ctx *, int n, const uint32_t *a_off, const uint32_t *b_off, const char *a, const char *b,
                uint32_t *out_off, uint32_t *out_len, char *out_a, char *out_b, size_t cap);
/* the same through each form of nw_alignment the kernels run: mode 0 = serial strips (what dg_probe_nw runs), 1 = register
 * strips (pairs up to 24 x 24), 2 = the wave-wide service (8-lane groups up to 64 columns, the whole wave beyond) with the
 * owner's traceback, 3 = the whole-wave form for every pair.  Modes 2 and 3 take the b side from a 2-bit text, as the
 * kernels do (RefSequence, bwt_index.cpp:193-212): b must be ACGT, else DG_ERR_ARG.                                  */
int dg_probe_nw_mode(dg_ctx *, int mode, int n, const uint32_t *a_off, const uint32_t *b_off, const char *a, const char *b,
                     uint32_t *out_off, uint32_t *out_len, char *out_a, char *out_b, size_t cap);
/* RefSequence[g0, g0 + n) (bwt_index.cpp:193-212) as the kernels read it from the device's 2-bit text, which holds the forward strand and -- built once at
 * start-up -- its reverse complement: out[i] = 'A' 'C' 'G' 'T', or 0 where g0 + i is outside [0, 2 l_pac).  n up to 2^30. */
int dg_probe_refseq(dg_ctx *, int64_t g0, int64_t n, char *out);
/* Test hook: the code-length builder of the dynamic BGZF coder (DG_BAM_DYNAMIC) on a histogram of the caller's, in a one-workgroup kernel: len_out[i] =
 * the length of symbol i's Huffman code, none above `limit` (1..15), 0 exactly where freq[i] is 0; one used symbol gets length 1.  The same integers as the
 * host's build of dg_bgzf_dyn.h gives.  n_sym 1..320, every freq below 2^23, no more used symbols than 2^limit, else DG_ERR_ARG.  A strip's own
 * histogram practically never needs the cut to 15 bits; this call reaches it. */
int dg_probe_huff_lengths(dg_ctx *, const uint32_t *freq, int n_sym, int limit, uint8_t *len_out);
/* Measuring hook: dg_bgzf_compress_flags(DG_BGZF_DYNAMIC) on n > 0 bytes with the kernel's clocks on: cycles[p] = lane 0's shader clocks between the barriers
 * of phase p, summed over all strips and blocks: 0 parse + merge + histogram, 1 sort, 2 code lengths (serial), 3 canonical codes, 4 header + choice (serial),
 * 5 scan + emit, 6 table inserts, 7 the rest (load, CRC, trailer).  The bytes are the unprobed call's and lie where dg_batch_download_bam finds them. */
int dg_probe_bgzf_phases(dg_ctx *, const void *host_bytes, size_t n, uint64_t cycles[8], size_t *n_bytes, float *device_ms);

#ifdef __cplusplus
}
#endif
#endif
