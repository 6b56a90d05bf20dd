"""ctypes binding of libdartgpu.so (include/dartgpu.h) plus the index loader.

Python here is plumbing for tests and bench.py; the product's host program is the C++ `dart`
command line (dart_amd/csrc/host/).  There is no CPU fallback: if libdartgpu.so is missing or no
HIP device is present, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DARTGPU_LIB") or os.path.join(_HERE, "libdartgpu.so")      # (DARTGPU_LIB: another build of the library, for A/B runs)


class IndexView(C.Structure):
    _fields_ = [("bwt", C.c_void_p), ("bwt_words", C.c_uint64), ("primary", C.c_uint64), ("L2", C.c_uint64 * 5),
                ("seq_len", C.c_uint64), ("sa", C.c_void_p), ("n_sa", C.c_uint64), ("sa_intv", C.c_int32),
                ("pac", C.c_void_p), ("l_pac", C.c_int64), ("n_chr", C.c_int32), ("chr_off", C.c_void_p),
                ("chr_len", C.c_void_p)]


class Params(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("max_gaps", "max_dup", "max_intron", "min_intron", "max_mismatch",
                                          "multi_hit", "all_sj", "paired")]


READ_OUT = np.dtype([("score", "<i4"), ("sub_score", "<i4"), ("mis_num", "<i4"), ("mapq", "<i4"), ("n_rep", "<i4"),
                     ("best", "<i4"), ("rep_off", "<i4"), ("sj_off", "<i4"), ("n_sj", "<i4")])
REPORT_OUT = np.dtype([("aln_score", "<i4"), ("sj_type", "<i4"), ("flag", "<i4"), ("paired_idx", "<i4"), ("chr", "<i4"),
                       ("bdir", "<i4"), ("pos", "<i8"), ("cigar_off", "<u4"), ("n_cigar", "<u4")])
SJ_OUT = np.dtype([("g1", "<i8"), ("g2", "<i8"), ("type", "<i4"), ("read_idx", "<i4")])
READ_C = np.dtype([("score", "<u2"), ("sub_score", "<u2"), ("mis_num", "<u2"), ("mapq", "u1"), ("n_sj", "u1"), ("n_rep", "<u2"), ("best", "<u2")])
REPORT_C = np.dtype([("pos", "<i4"), ("aln_score", "<u2"), ("flag", "<u2"), ("paired_idx", "<i2"), ("chr", "<u2"), ("n_cigar", "u1"),
                     ("sj_type", "i1"), ("bdir", "u1"), ("pad", "u1")])
CIGAR_FULL_MATCH = 255
SJ_ENTRY = np.dtype([("g1", "<i8"), ("g2", "<i8"), ("count", "<u4"), ("chr", "<u4")])      # dg_sj_entry
SJ_ENTRIES_ONLY = 1
COV_ENTRY = np.dtype([("chr", "<u4"), ("start", "<u4"), ("end", "<u4"), ("depth", "<u4")])      # dg_cov_entry
COV_ENTRIES_ONLY, COV_STRAND_PLUS, COV_STRAND_MINUS = 1, 2, 4
SITE_ENTRY = np.dtype([("chr", "<u4"), ("pos", "<u4"), ("depth", "<u4"), ("depth_rev", "<u4"), ("ref", "<u4"), ("top", "<u4"), ("n", "<u4", (7,)), ("n_rev", "<u4", (7,))])      # dg_site_entry
PU_ENTRIES_ONLY = 1
MD_COUNT_ONLY = 1                                                                                 # DG_MD_COUNT_ONLY
TAG_MD, TAG_NM, TAG_TS = 1, 2, 4                                                                  # DG_TAG_*
SJ_NO_CHR = 0xFFFFFFFF
GENE_EXON = np.dtype([("chr", "<i4"), ("start", "<u4"), ("end", "<u4"), ("strand", "<u4"), ("gene", "<u4")])      # dg_gene_exon
GENE_NONE, GENE_AMBIG = 0xFFFFFFFF, 0xFFFFFFFE


class DgUmi(C.Structure):                                                                         # dg_umi
    _fields_ = [("flags", C.c_uint32), ("len", C.c_uint32 * 2), ("skip", C.c_uint32 * 2), ("sep", C.c_char), ("pad", C.c_char * 3)]


class DgUmiRules(C.Structure):                                                                    # dg_umi_rules
    _fields_ = [("flags", C.c_uint32), ("max_edit", C.c_uint32), ("sep", C.c_char), ("pad", C.c_char * 3)]


class GeneAnnot(C.Structure):
    _fields_ = [("n_genes", C.c_uint32), ("pad", C.c_uint32), ("n_exons", C.c_size_t), ("exons", C.c_void_p)]


RNA_TX = np.dtype([("chr", "<i4"), ("strand", "<u4"), ("flags", "<u4"), ("cds_start", "<u4"), ("cds_end", "<u4"), ("n_exons", "<u4"), ("first_exon", "<u8")])      # dg_rna_tx
RNA_EXON = np.dtype([("start", "<u4"), ("end", "<u4")])                                           # dg_rna_exon
RNA_TX_RIBOSOMAL = 1                                                                              # DG_RNA_TX_RIBOSOMAL


class RnaAnnot(C.Structure):
    _fields_ = [("n_tx", C.c_uint32), ("pad", C.c_uint32), ("n_exons", C.c_size_t), ("tx", C.c_void_p), ("exons", C.c_void_p)]
assert READ_OUT.itemsize == 36 and REPORT_OUT.itemsize == 40 and SJ_OUT.itemsize == 24 and READ_C.itemsize == 12 and REPORT_C.itemsize == 16


def tx_text(lib, words, tx, exons, names) -> bytes:
    """the text of the expression stage's result words under the annotation they were made with (dg_tx_format: on the host, no context)"""
    w = np.ascontiguousarray(words, np.uint64); t = np.ascontiguousarray(tx, RNA_TX); e = np.ascontiguousarray(exons, RNA_EXON)
    ann = RnaAnnot(len(t), 0, len(e), t.ctypes.data if len(t) else None, e.ctypes.data if len(e) else None)
    arr = (C.c_char_p * max(len(names), 1))(*[n.encode() if isinstance(n, str) else n for n in names])
    nb = C.c_size_t(0)
    rc = lib.dg_tx_format(w.ctypes.data, len(w), C.byref(ann), arr, None, 0, C.byref(nb))
    if rc not in (0, -4):
        raise RuntimeError("dg_tx_format failed (%d)" % rc)
    out = C.create_string_buffer(max(nb.value, 1))
    rc = lib.dg_tx_format(w.ctypes.data, len(w), C.byref(ann), arr, out, nb.value, C.byref(nb))
    if rc != 0:
        raise RuntimeError("dg_tx_format failed (%d)" % rc)
    return out.raw[:nb.value]


def expand_compact(reads_c, reports_c, cigar_c, rlen):
    """dg_read_c / dg_report_c arrays + the stored CIGAR ops + the read lengths -> (reads, reports, cigar ops) in the full record
    dtypes: rep_off / sj_off as running sums; a report marked DG_CIGAR_FULL_MATCH gets its "<length of its read>M" back; the stored ops
    lie in two regions (include/dartgpu.h): first, report by report, those of the reports with pad bit 0 clear, then those of the
    reports with it set -- a report's ops start at the running sum of the stored counts inside its region.  The reference expansion
    of the compact layout."""
    n = len(reads_c)
    r = np.zeros(n, READ_OUT)
    for f in ("score", "sub_score", "mis_num", "mapq", "n_rep", "best", "n_sj"):
        r[f] = reads_c[f]
    nrep = reads_c["n_rep"].astype(np.int64)
    r["rep_off"] = np.cumsum(nrep) - nrep
    nsj = reads_c["n_sj"].astype(np.int64)
    r["sj_off"] = np.cumsum(nsj) - nsj
    m = len(reports_c)
    assert m == int(nrep.sum()), "the reports do not add up to the reads' n_rep"
    p = np.zeros(m, REPORT_OUT)
    for f in ("aln_score", "sj_type", "flag", "paired_idx", "bdir", "pos"):
        p[f] = reports_c[f]
    p["chr"] = np.where(reports_c["chr"] == 0xFFFF, -1, reports_c["chr"].astype(np.int32))
    plain = reports_c["n_cigar"] == CIGAR_FULL_MATCH
    second = (reports_c["pad"] & 1) != 0
    stored = np.where(plain, 0, reports_c["n_cigar"]).astype(np.int64)
    full = np.where(plain, 1, reports_c["n_cigar"]).astype(np.int64)
    p["n_cigar"] = full
    off_full = np.cumsum(full) - full
    p["cigar_off"] = off_full
    cig = np.zeros(int(full.sum()), np.uint32)
    owner = np.repeat(np.arange(n), nrep)                         # the read of every report
    cig[off_full[plain]] = np.asarray(rlen, np.uint32)[owner[plain]] << 4
    # where a report's stored ops start: the running sum inside its region; the second region begins behind the whole first one
    s1 = np.where(second, 0, stored); s2 = np.where(second, stored, 0)
    src = np.where(second, int(s1.sum()) + np.cumsum(s2) - s2, np.cumsum(s1) - s1)
    sel = stored > 0
    if sel.any():
        st = stored[sel]
        k = np.arange(int(st.sum())) - np.repeat(np.cumsum(st) - st, st)
        cig[np.repeat(off_full[sel], st) + k] = np.asarray(cigar_c, np.uint32)[np.repeat(src[sel], st) + k]
    return r, p, cig


class IndexFiles(C.Structure):
    _fields_ = [("bwt_path", C.c_char_p), ("sa_path", C.c_char_p), ("pac_path", C.c_char_p), ("l_pac", C.c_int64), ("n_chr", C.c_int32),
                ("chr_off", C.c_void_p), ("chr_len", C.c_void_p), ("expected_reads", C.c_uint64)]


INIT_ASYNC_AIDS = 1


class SamText(C.Structure):
    _fields_ = [("hdr_off", C.c_void_p), ("hdr", C.c_void_p), ("qual_off", C.c_void_p), ("qual", C.c_void_p), ("n_pair_mode", C.c_int32)]


SAM_UNIQUE_ONLY = 1
BAM_RAW = 2
BAM_DYNAMIC = 4            # DG_BAM_DYNAMIC: BGZF with dynamic Huffman codes per strip
BGZF_DYNAMIC = 1           # DG_BGZF_DYNAMIC: the same for dg_bgzf_compress_flags


class FastqText(C.Structure):
    _fields_ = [("text1", C.c_void_p), ("n1", C.c_size_t), ("text2", C.c_void_p), ("n2", C.c_size_t), ("rc_odd_reads", C.c_int32), ("max_reads", C.c_int32)]


class FastqBgzf(C.Structure):
    _fields_ = [("head1", C.c_void_p), ("n_head1", C.c_size_t), ("blocks1", C.c_void_p), ("n_blocks1", C.c_size_t),
                ("head2", C.c_void_p), ("n_head2", C.c_size_t), ("blocks2", C.c_void_p), ("n_blocks2", C.c_size_t),
                ("rc_odd_reads", C.c_int32), ("max_reads", C.c_int32), ("last", C.c_int32)]


FQ_CHECK_ONLY = 1           # DG_FQ_CHECK_ONLY: inflate, count and check; no batch is written


class Trim(C.Structure):
    """dg_trim (include/dartgpu.h)"""
    _fields_ = [("flags", C.c_uint32), ("qual3", C.c_uint32), ("qual5", C.c_uint32), ("qual_base", C.c_uint32), ("min_overlap", C.c_uint32), ("max_err_permille", C.c_uint32),
                ("poly_mask", C.c_uint32), ("poly_min", C.c_uint32), ("min_len", C.c_uint32), ("n_adapter", C.c_uint32 * 2), ("adapter", (C.c_char * 64) * 2)]


TRIM_PAIRS = 1              # DG_TRIM_PAIRS: reads 2k and 2k+1 are mates
TRIM_STAT_KEYS = ("reads_in", "reads_kept", "bases_in", "bases_kept", "qual5_bases", "qual3_bases", "adapter0_reads", "adapter1_reads", "adapter_bases", "poly_reads",
                  "poly_bases", "too_short_reads", "mate_dropped_reads", "qual_skipped_reads")


def flatten_strings(items):
    """list of bytes / str -> (u32 offsets [n + 1], u8 array): the form dg_set_chr_names and dg_batch_format_sam take names and qualities in"""
    bs = [x if isinstance(x, (bytes, bytearray)) else x.encode("latin1") for x in items]
    off = np.zeros(len(bs) + 1, np.uint32)
    if bs:
        off[1:] = np.cumsum([len(x) for x in bs])
    return off, np.frombuffer(b"".join(bs) + b"\0", np.uint8).copy()


class Index:
    """The BWA-format index files as the reference loads them (bwt_index.cpp:15-35,102-121,229-251).  The headers and the chromosome
    table are read at once; the three big arrays only when something asks for them (dg_init's host-array view, tests): dg_init_files
    takes them from the files straight to HBM."""

    def __init__(self, prefix: str):
        self.prefix = prefix
        hdr = np.fromfile(prefix + ".bwt", dtype=np.uint64, count=5)
        self.primary = int(hdr[0])
        self.L2 = [0] + [int(x) for x in hdr[1:5]]
        self.seq_len = self.L2[4]
        sa_hdr = np.fromfile(prefix + ".sa", dtype=np.uint64, count=7)
        self.sa_intv = int(sa_hdr[5])
        self.n_sa = (self.seq_len + self.sa_intv) // self.sa_intv
        self._bwt = self._sa = self._pac = None
        with open(prefix + ".ann") as f:
            first = f.readline().split()
            self.l_pac, n = int(first[0]), int(first[1])
            self.names, lens = [], []
            for _ in range(n):
                self.names.append(f.readline().split()[1])
                lens.append(int(f.readline().split()[1]))
        self.chr_len = np.asarray(lens, dtype=np.int64)
        self.chr_off = np.concatenate([[0], np.cumsum(self.chr_len)[:-1]]).astype(np.int64)

    @property
    def bwt(self):
        if self._bwt is None:
            self._bwt = np.fromfile(self.prefix + ".bwt", dtype=np.uint32, offset=40)
        return self._bwt

    @property
    def sa(self):
        if self._sa is None:
            sa = np.zeros(self.n_sa, dtype=np.uint64)
            sa[0] = np.uint64(0xFFFFFFFFFFFFFFFF)
            body = np.fromfile(self.prefix + ".sa", dtype=np.uint64, offset=56, count=self.n_sa - 1)
            sa[1:1 + len(body)] = body
            self._sa = sa
        return self._sa

    @property
    def pac(self):
        if self._pac is None:
            self._pac = np.fromfile(self.prefix + ".pac", dtype=np.uint8)
        return self._pac

    def files(self, expected_reads: int = 0) -> IndexFiles:
        f = IndexFiles()
        f.expected_reads = int(expected_reads)
        self._paths = [(self.prefix + e).encode() for e in (".bwt", ".sa", ".pac")]
        f.bwt_path, f.sa_path, f.pac_path = self._paths
        f.l_pac = self.l_pac; f.n_chr = len(self.names)
        f.chr_off = self.chr_off.ctypes.data; f.chr_len = self.chr_len.ctypes.data
        return f

    def view(self) -> IndexView:
        v = IndexView()
        v.bwt = self.bwt.ctypes.data; v.bwt_words = self.bwt.size; v.primary = self.primary
        for i in range(5):
            v.L2[i] = self.L2[i]
        v.seq_len = self.seq_len; v.sa = self.sa.ctypes.data; v.n_sa = self.n_sa; v.sa_intv = self.sa_intv
        v.pac = self.pac.ctypes.data; v.l_pac = self.l_pac; v.n_chr = len(self.names)
        v.chr_off = self.chr_off.ctypes.data; v.chr_len = self.chr_len.ctypes.data
        return v


def pack_reads(seqs):
    """list of bytes / 2-D uint8 array -> (seq_off u32, rlen u16, flat uint8)."""
    if isinstance(seqs, np.ndarray) and seqs.ndim == 2:
        n, l = seqs.shape
        return (np.arange(n, dtype=np.uint32) * np.uint32(l)), np.full(n, l, dtype=np.uint16), np.ascontiguousarray(seqs).reshape(-1)
    lens = np.asarray([len(s) for s in seqs], dtype=np.uint16)
    off = np.concatenate([[0], np.cumsum(lens.astype(np.int64))[:-1]]).astype(np.uint32) if len(seqs) else np.zeros(0, np.uint32)
    flat = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy() if len(seqs) else np.zeros(0, np.uint8)
    return off, lens, flat


def interleave_pairs(m1: np.ndarray, m2: np.ndarray) -> np.ndarray:
    """mate 1 rows / mate 2 rows -> [2n, rlen] with mate 2 reverse-complemented the way the
    reference's loader does (GetData.cpp:157-162: anything but ACGT/acgt becomes 'N')."""
    comp = np.full(256, ord("N"), dtype=np.uint8)
    for a, b in zip(b"ACGTacgt", b"TGCATGCA"):
        comp[a] = b
    out = np.empty((2 * m1.shape[0], m1.shape[1]), dtype=np.uint8)
    out[0::2] = m1
    out[1::2] = comp[m2[:, ::-1]]
    return out


def _load_lib():
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libdartgpu.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                           "there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    lib.dg_init.restype = C.c_void_p
    lib.dg_init.argtypes = [C.POINTER(IndexView), C.POINTER(Params), C.c_int, C.POINTER(C.c_int)]
    lib.dg_init_files.restype = C.c_void_p
    lib.dg_init_files.argtypes = [C.POINTER(IndexFiles), C.POINTER(Params), C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.dg_index_wait.argtypes = [C.c_void_p]
    lib.dg_init_report.restype = C.c_char_p
    lib.dg_init_report.argtypes = [C.c_void_p]
    lib.dg_device_count.restype = C.c_int
    lib.dg_last_error.restype = C.c_char_p
    lib.dg_last_error.argtypes = [C.c_void_p]
    lib.dg_destroy.argtypes = [C.c_void_p]
    lib.dg_clone.restype = C.c_void_p
    lib.dg_clone.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.dg_set_params.argtypes = [C.c_void_p, C.POINTER(Params)]
    lib.dg_params_default.argtypes = [C.POINTER(Params)]
    vp = C.c_void_p
    lib.dg_map_batch.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.dg_batch_upload.argtypes = [vp, C.c_int, vp, vp, vp]
    lib.dg_batch_upload_packed.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, C.c_size_t]
    lib.dg_map_batch_packed.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, C.c_size_t, vp, vp, vp, vp, vp, vp]
    lib.dg_batch_download_compact.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.dg_map_batch_compact.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_size_t, vp, vp, vp, vp, vp, vp]
    lib.dg_host_alloc.restype = C.c_void_p
    lib.dg_host_alloc.argtypes = [C.c_size_t]
    lib.dg_host_free.argtypes = [vp]
    lib.dg_batch_run.argtypes = [vp, vp]
    lib.dg_batch_download.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.dg_batch_device_ptrs.argtypes = [vp, vp]
    lib.dg_batch_device_ptrs_compact.argtypes = [vp, vp]
    if hasattr(lib, "dg_batch_device_records_compact"):      # (absent from older builds of the library loaded through DARTGPU_LIB for A/B runs)
        lib.dg_batch_device_records_compact.argtypes = [vp, vp, vp]
    lib.dg_last_timings.argtypes = [vp, vp, vp, C.c_int]
    if hasattr(lib, "dg_batch_format_sam"):                  # (likewise: the device's SAM formatter)
        lib.dg_set_chr_names.argtypes = [vp, C.c_int, vp, vp]
        lib.dg_batch_format_sam.argtypes = [vp, vp, C.c_uint32, vp, vp, vp]
        lib.dg_batch_download_sam.argtypes = [vp, vp, C.c_size_t]
        lib.dg_batch_device_sam.argtypes = [vp, vp, vp]
    if hasattr(lib, "dg_batch_upload_fastq"):
        lib.dg_batch_upload_fastq.argtypes = [vp, vp, vp]
        lib.dg_batch_format_sam_resident.argtypes = [vp, C.c_int, C.c_uint32, vp, vp, vp]
        lib.dg_batch_download_reads.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.dg_batch_fastq_device_ms.argtypes = [vp, vp]
        lib.dg_fastq_tile.restype = C.c_int
    if hasattr(lib, "dg_set_trim"):                          # (likewise: trimming inside the FASTQ upload)
        lib.dg_set_trim.argtypes = [vp, vp]
        lib.dg_batch_trim_stats.argtypes = [vp, vp, vp]
        lib.dg_trim_granules.argtypes = [vp]
    if hasattr(lib, "dg_set_umi"):                           # (likewise: inline UMIs cut inside the FASTQ upload)
        lib.dg_set_umi.argtypes = [vp, vp]
    if hasattr(lib, "dg_batch_format_bam"):                  # (likewise: BAM records and BGZF blocks on the device)
        lib.dg_batch_format_bam.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, vp]
        lib.dg_batch_format_bam_resident.argtypes = [vp, C.c_int, C.c_uint32, vp, vp, vp, vp]
        lib.dg_batch_download_bam.argtypes = [vp, vp, C.c_size_t]
        lib.dg_batch_device_bam.argtypes = [vp, vp, vp]
        lib.dg_bgzf_compress.argtypes = [vp, vp, C.c_size_t, vp, vp]
        lib.dg_bgzf_granules.argtypes = [vp]
    if hasattr(lib, "dg_bgzf_compress_flags"):
        lib.dg_bgzf_compress_flags.argtypes = [vp, vp, C.c_size_t, C.c_uint32, vp, vp]
        lib.dg_probe_huff_lengths.argtypes = [vp, vp, C.c_int, C.c_int, vp]
        lib.dg_probe_bgzf_phases.argtypes = [vp, vp, C.c_size_t, vp, vp, vp]
        lib.dg_batch_bam_device_ms.argtypes = [vp, vp]
    if hasattr(lib, "dg_bgzf_inflate"):                      # (likewise: BGZF inflated on the device, in front of the FASTQ parser)
        lib.dg_bgzf_inflate.argtypes = [vp, vp, C.c_size_t, vp, vp, vp]
        lib.dg_inflate_download.argtypes = [vp, vp, C.c_size_t]
        lib.dg_inflate_device.argtypes = [vp, vp, vp]
        lib.dg_batch_upload_fastq_bgzf.argtypes = [vp, vp, C.c_uint32, vp, vp, vp]
        lib.dg_batch_download_fastq_tail.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t]
        lib.dg_inflate_granules.argtypes = [vp]
    if hasattr(lib, "dg_sj_finish"):                         # (likewise: the splice-junction table on the device)
        lib.dg_sj_reserve.argtypes = [vp, C.c_size_t]
        lib.dg_sj_reset.argtypes = [vp]
        lib.dg_batch_accumulate_sj.argtypes = [vp, vp]
        lib.dg_sj_add.argtypes = [vp, vp, C.c_size_t]
        lib.dg_sj_merge.argtypes = [vp, vp]
        lib.dg_sj_finish.argtypes = [vp, C.c_uint32, vp, vp, vp, vp]
        lib.dg_sj_download.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t]
        lib.dg_sj_device.argtypes = [vp, vp, vp]
        lib.dg_sj_granules.argtypes = [vp]
    if hasattr(lib, "dg_bam_sort_finish"):                   # (likewise: coordinate-sorted BAM on the device)
        lib.dg_batch_accumulate_bam.argtypes = [vp, C.c_uint32, vp, vp]
        lib.dg_bam_sort_add.argtypes = [vp, vp, C.c_size_t, C.c_uint32, vp]
        lib.dg_bam_sort_merge.argtypes = [vp, vp]
        lib.dg_bam_sort_reset.argtypes = [vp]
        lib.dg_bam_sort_finish.argtypes = [vp, vp, vp, vp]
        lib.dg_bam_sort_device_ms.argtypes = [vp, vp, vp]
        lib.dg_bam_sort_device.argtypes = [vp, vp, vp]
        lib.dg_bam_sort_compress.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_uint32, vp, vp]
        lib.dg_bam_sort_granules.argtypes = [vp]
        lib.dg_bam_sort_info.argtypes = [vp, vp]                # (a test hook, not in include/dartgpu.h)
    if hasattr(lib, "dg_bam_index_finish"):                  # (likewise: the BAM index of the sorted array)
        lib.dg_bam_index_finish.argtypes = [vp, C.c_uint64, vp, C.c_size_t, vp, vp, vp]
        lib.dg_bam_index_download.argtypes = [vp, vp, C.c_size_t]
        lib.dg_bam_index_device.argtypes = [vp, vp, vp]
        lib.dg_bam_index_granules.argtypes = [vp]
    if hasattr(lib, "dg_bam_coverage_finish"):               # (likewise: the coverage track of the sorted array)
        lib.dg_bam_coverage_finish.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
        lib.dg_bam_coverage_download.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t]
        lib.dg_bam_coverage_device.argtypes = [vp, vp, vp]
        lib.dg_bam_coverage_device_ms.argtypes = [vp, vp, vp]
        lib.dg_bam_coverage_granules.argtypes = [vp]
    if hasattr(lib, "dg_bam_pileup_finish"):                 # (likewise: the allele counts of the sorted array)
        lib.dg_bam_pileup_finish.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
        lib.dg_bam_pileup_download.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t]
        lib.dg_bam_pileup_device.argtypes = [vp, vp, vp]
        lib.dg_bam_pileup_device_ms.argtypes = [vp, vp, vp]
        lib.dg_bam_pileup_granules.argtypes = [vp]
    if hasattr(lib, "dg_bam_qc_finish"):                     # (likewise: the QC tables of the sorted array)
        lib.dg_bam_qc_finish.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
        lib.dg_bam_qc_download.argtypes = [vp, vp, C.c_size_t]
        lib.dg_bam_qc_device.argtypes = [vp, vp]
        lib.dg_bam_qc_device_ms.argtypes = [vp, vp]
        lib.dg_bam_qc_granules.argtypes = [vp]
        lib.dg_bam_qc_offsets.argtypes = [C.c_int, vp]
        lib.dg_bam_qc_format.argtypes = [vp, C.c_size_t, C.c_int, vp, vp, vp, C.c_size_t, vp]
    if hasattr(lib, "dg_bam_markdup_finish"):                # (likewise: duplicate marking of the sorted array)
        lib.dg_bam_markdup_finish.argtypes = [vp, C.c_uint32, vp, vp]
        lib.dg_bam_markdup_device_ms.argtypes = [vp, vp, vp]
        lib.dg_bam_markdup_granules.argtypes = [vp]
    if hasattr(lib, "dg_bam_markdup_umi_finish"):            # (likewise: UMI-aware duplicate marking)
        lib.dg_bam_markdup_umi_finish.argtypes = [vp, vp, C.c_uint32, vp, vp]
        lib.dg_bam_markdup_umi_device_ms.argtypes = [vp, vp, vp]
        lib.dg_bam_markdup_umi_granules.argtypes = [vp]
    if hasattr(lib, "dg_bam_tags_finish"):                   # (likewise: MD / NM / ts on the sorted array)
        lib.dg_bam_tags_finish.argtypes = [vp, C.c_uint32, vp, vp, vp]
        lib.dg_bam_tags_device_ms.argtypes = [vp, vp]
        lib.dg_bam_tags_granules.argtypes = [vp]
        lib.dg_bam_tags_write_ms.argtypes = [vp, vp]                # (a probe's hook, not in include/dartgpu.h)
    if hasattr(lib, "dg_bam_rna_finish"):                    # (likewise: the RNA-seq metrics of the sorted array)
        lib.dg_rna_set_annotation.argtypes = [vp, vp, vp, vp]
        lib.dg_bam_rna_finish.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp]
        lib.dg_bam_rna_download.argtypes = [vp, vp, C.c_size_t]
        lib.dg_bam_rna_device.argtypes = [vp, vp]
        lib.dg_bam_rna_device_ms.argtypes = [vp, vp]
        lib.dg_bam_rna_granules.argtypes = [vp]
        lib.dg_bam_rna_offsets.argtypes = [vp]
        lib.dg_bam_rna_format.argtypes = [vp, C.c_size_t, vp, C.c_size_t, vp]
    if hasattr(lib, "dg_gene_set_annotation"):               # (likewise: gene-level read counts)
        lib.dg_gene_set_annotation.argtypes = [vp, vp, vp]
        lib.dg_batch_accumulate_genes.argtypes = [vp, C.c_int, C.c_uint32, vp]
        lib.dg_gene_count_records.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, vp, vp, C.c_size_t, vp, C.c_size_t, vp]
        lib.dg_gene_add.argtypes = [vp, vp, C.c_size_t]
        lib.dg_gene_merge.argtypes = [vp, vp]
        lib.dg_gene_reset.argtypes = [vp]
        lib.dg_gene_download.argtypes = [vp, vp, C.c_size_t]
        lib.dg_gene_device.argtypes = [vp, vp]
        lib.dg_gene_device_ms.argtypes = [vp, vp]
        lib.dg_gene_granules.argtypes = [vp]
    if hasattr(lib, "dg_tx_set_annotation"):                 # (likewise: transcript-level expression)
        lib.dg_tx_set_annotation.argtypes = [vp, vp, vp, vp]
        lib.dg_batch_accumulate_tx.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, vp]
        lib.dg_tx_count_records.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, vp, vp, C.c_size_t, vp, C.c_size_t, vp]
        lib.dg_tx_merge.argtypes = [vp, vp]
        lib.dg_tx_add.argtypes = [vp, vp, vp, vp, C.c_size_t, vp]
        lib.dg_tx_reset.argtypes = [vp]
        lib.dg_tx_classes_size.argtypes = [vp, vp, vp]
        lib.dg_tx_classes_download.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_size_t, vp]
        lib.dg_tx_finish.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint32, vp, vp]
        lib.dg_tx_download.argtypes = [vp, vp, C.c_size_t]
        lib.dg_tx_device.argtypes = [vp, vp, vp]
        lib.dg_tx_device_ms.argtypes = [vp, vp]
        lib.dg_tx_granules.argtypes = [vp]
        lib.dg_tx_format.argtypes = [vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp]
    lib.dg_last_counters.argtypes = [vp, vp, C.c_int]
    lib.dg_probe_seeds.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    lib.dg_probe_nw.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t]
    lib.dg_probe_nw_mode.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t]
    lib.dg_probe_refseq.argtypes = [vp, C.c_int64, C.c_int64, vp]
    return lib


def pack_reads_2bit(arr: np.ndarray):
    """[n, rlen] uint8 ASCII (A/C/G/T/N upper case only) -> (words u32 [n, ceil(rlen/16)], nlist u32) for dg_map_batch_packed:
    16 bases per word, first base in the top bits; N stored as A and listed as flat index i * 16 * W + pos."""
    n, l = arr.shape
    W = (l + 15) // 16
    code = np.full(256, 255, np.uint8)
    for ch, v in zip(b"ACGTN", (0, 1, 2, 3, 0)):
        code[ch] = v
    c = code[arr]
    if (c == 255).any():
        raise ValueError("packed reads hold A, C, G, T, N only")
    padded = np.zeros((n, 16 * W), np.uint32)
    padded[:, :l] = c
    sh = (30 - 2 * np.arange(16, dtype=np.uint32))
    words = (padded.reshape(n, W, 16) << sh).sum(axis=2, dtype=np.uint64).astype(np.uint32)
    ri, pi = np.nonzero(arr == ord("N"))
    nlist = (ri.astype(np.uint64) * (16 * W) + pi.astype(np.uint64)).astype(np.uint32)
    return np.ascontiguousarray(words), nlist


class PinnedArray:
    """numpy view of page-locked host memory (dg_host_alloc): copies to/from it are DMA transfers"""

    def __init__(self, lib, shape, dtype):
        self.lib = lib
        dt = np.dtype(dtype)
        n = int(np.prod(shape))
        self.ptr = lib.dg_host_alloc(max(n * dt.itemsize, 64))
        if not self.ptr:
            raise MemoryError("dg_host_alloc failed")
        buf = (C.c_char * (n * dt.itemsize)).from_address(self.ptr)
        self.a = np.frombuffer(buf, dtype=dt, count=n).reshape(shape)

    def free(self):
        if self.ptr:
            self.a = None
            self.lib.dg_host_free(self.ptr)
            self.ptr = None


def default_params(**kw) -> Params:
    p = Params(5, 100, 500000, 5, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(p, k, int(v))
    return p


class BatchResult:
    def __init__(self, reads, reports, cigar, sj):
        self.reads, self.reports, self.cigar, self.sj = reads, reports, cigar, sj

    def cigar_string(self, rep_index: int) -> str:
        r = self.reports[rep_index]
        ops = self.cigar[r["cigar_off"]: r["cigar_off"] + r["n_cigar"]]
        return "".join("%d%s" % (o >> 4, "MIDNS"[o & 15]) for o in ops)


QC_SECTIONS = (("FS", (2, 16)), ("CH", None), ("MQ", (256,)), ("IS", (3, 8001)), ("RL", (2, 512)), ("PC", (2, 12, 512)), ("ID", (2, 65)), ("SN", (32,)))


def qc_views(lib, words, n_chr: int):
    """the flat QC words (dg_bam_qc_download) sliced into named views by dg_bam_qc_offsets"""
    off = (C.c_size_t * 9)()
    if lib.dg_bam_qc_offsets(int(n_chr), off) != 0 or int(off[8]) != len(words):
        raise RuntimeError("dg_bam_qc_offsets: %d words do not fit %d chromosomes" % (len(words), n_chr))
    out = {"words": words}
    for k, (name, shape) in enumerate(QC_SECTIONS):
        out[name] = words[int(off[k]):int(off[k + 1])].reshape(shape if shape else (n_chr + 1, 2))
    return out


def qc_text(lib, words, names, lengths) -> bytes:
    """dg_bam_qc_format: the text of the flat QC words; needs no device"""
    w = np.ascontiguousarray(words, np.uint64)
    nm = [n if isinstance(n, bytes) else n.encode() for n in names]
    arr = (C.c_char_p * len(nm))(*nm)
    ln = np.ascontiguousarray(lengths, np.int64)
    nb = C.c_size_t(0)
    rc = lib.dg_bam_qc_format(w.ctypes.data, len(w), len(nm), arr, ln.ctypes.data, None, 0, C.byref(nb))
    if rc not in (0, -4):
        raise RuntimeError("dg_bam_qc_format failed (%d)" % rc)
    buf = np.zeros(max(int(nb.value), 1), np.uint8)
    rc = lib.dg_bam_qc_format(w.ctypes.data, len(w), len(nm), arr, ln.ctypes.data, buf.ctypes.data, int(nb.value), C.byref(nb))
    if rc != 0:
        raise RuntimeError("dg_bam_qc_format failed (%d)" % rc)
    return buf[:int(nb.value)].tobytes()


RNA_SECTIONS = (("BA", (5,)), ("RC", (5,)), ("ST", (4,)), ("BC", (3, 100)), ("SN", (16,)))


def rna_views(lib, words):
    """the flat RNA-metrics words (dg_bam_rna_download) sliced into named views by dg_bam_rna_offsets"""
    off = (C.c_size_t * 6)()
    if lib.dg_bam_rna_offsets(off) != 0 or int(off[5]) != len(words):
        raise RuntimeError("dg_bam_rna_offsets: %d words where %d are expected" % (len(words), int(off[5])))
    out = {"words": words}
    for k, (name, shape) in enumerate(RNA_SECTIONS):
        out[name] = words[int(off[k]):int(off[k + 1])].reshape(shape)
    return out


def rna_text(lib, words) -> bytes:
    """dg_bam_rna_format: the text of the flat RNA-metrics words (or of a dict of rna_views); needs no device"""
    w = np.ascontiguousarray(words["words"] if isinstance(words, dict) else words, np.uint64)
    nb = C.c_size_t(0)
    rc = lib.dg_bam_rna_format(w.ctypes.data, len(w), None, 0, C.byref(nb))
    if rc not in (0, -4):
        raise RuntimeError("dg_bam_rna_format failed (%d)" % rc)
    buf = np.zeros(max(int(nb.value), 1), np.uint8)
    rc = lib.dg_bam_rna_format(w.ctypes.data, len(w), buf.ctypes.data, int(nb.value), C.byref(nb))
    if rc != 0:
        raise RuntimeError("dg_bam_rna_format failed (%d)" % rc)
    return buf[:int(nb.value)].tobytes()


class DartGPU:
    """dg_ctx wrapper: DART's per-read mapping path on one MI355X."""

    def __init__(self, index: Index, params: Params | None = None, device: int = 0, from_files: bool | None = None, async_aids: bool = False, expected_reads: int = 0):
        """from_files (default: unless DART_INIT_VIEW=1): dg_init_files -- the index files go straight to HBM; False: dg_init with the
        host-array view.  async_aids: the look-up aids are built in the background (dg_index_wait / wait_index joins them)."""
        self.lib = _load_lib()
        self.index = index
        self.params = params or default_params()
        st = C.c_int(0)
        if from_files is None:
            from_files = os.environ.get("DART_INIT_VIEW") != "1"
        if from_files:
            f = index.files(expected_reads)      # (expected_reads: 0 = unknown -> full aids; a short job gets lean ones)
            self.ctx = self.lib.dg_init_files(C.byref(f), C.byref(self.params), device, INIT_ASYNC_AIDS if async_aids else 0, C.byref(st))
        else:
            v = index.view()
            self.ctx = self.lib.dg_init(C.byref(v), C.byref(self.params), device, C.byref(st))
        if not self.ctx:
            raise RuntimeError("dg_init failed (%d): %s" % (st.value, (self.lib.dg_last_error(None) or b"").decode()))
        if hasattr(self.lib, "dg_set_chr_names"):            # (an older build loaded through DARTGPU_LIB has no formatter: format_sam then raises)
            self.set_chr_names(index.names)

    def set_chr_names(self, names):
        """the chromosome names the device's SAM formatter prints (dg_set_chr_names): kept with the index, shared by clones"""
        off, flat = flatten_strings(names)
        self._chk(self.lib.dg_set_chr_names(self.ctx, len(names), off.ctypes.data, flat.ctypes.data), "dg_set_chr_names")

    def format_sam(self, headers, quals, n_pair_mode: int, unique_only: bool = False):
        """SAM text of the batch that ran last, formatted on the device (dg_batch_format_sam + dg_batch_download_sam) -> (bytes, counters);
        headers / quals: one bytes or str per read, qualities in stored order (mate 2's reversed), quals None = FASTA ('*');
        counters: dict unmapped / unique / paired; self.sam_device_ms holds the kernels' device time"""
        if not hasattr(self.lib, "dg_batch_format_sam"):
            raise RuntimeError("this build of libdartgpu.so has no dg_batch_format_sam")
        ho, hb = flatten_strings(headers)
        t = SamText()
        t.hdr_off, t.hdr, t.n_pair_mode = ho.ctypes.data, hb.ctypes.data, int(n_pair_mode)
        if quals is not None:
            qo, qb = flatten_strings(quals)
            t.qual_off, t.qual = qo.ctypes.data, qb.ctypes.data
        nb = C.c_size_t(0); ct = (C.c_uint64 * 3)(); ms = C.c_float(0)
        self._chk(self.lib.dg_batch_format_sam(self.ctx, C.byref(t), SAM_UNIQUE_ONLY if unique_only else 0, C.byref(nb), ct, C.byref(ms)), "dg_batch_format_sam")
        self.sam_device_ms = float(ms.value)
        out = np.zeros(max(int(nb.value), 1), np.uint8)
        self._chk(self.lib.dg_batch_download_sam(self.ctx, out.ctypes.data, int(nb.value)), "dg_batch_download_sam")
        return out[:int(nb.value)].tobytes(), dict(unmapped=int(ct[0]), unique=int(ct[1]), paired=int(ct[2]))

    def fastq_tile(self) -> int:
        """bytes of FASTQ text one workgroup of the device parser's line kernels takes (dg_fastq_tile)"""
        return int(self.lib.dg_fastq_tile())

    def upload_fastq(self, text1, text2=None, rc_odd_reads: bool = False, max_reads: int | None = None) -> int:
        """FASTQ bytes -> the batch in HBM (dg_batch_upload_fastq); two texts: reads alternate between them.  Returns the number of reads.
        max_reads None: as many as the texts can hold.  self.fastq_device_ms holds the six kernels' device time."""
        if not hasattr(self.lib, "dg_batch_upload_fastq"):
            raise RuntimeError("this build of libdartgpu.so has no dg_batch_upload_fastq")
        a = np.frombuffer(bytes(text1) + b"\0", np.uint8)
        b = np.frombuffer(bytes(text2) + b"\0", np.uint8) if text2 is not None else None
        t = FastqText()
        t.text1, t.n1 = a.ctypes.data, len(a) - 1
        if b is not None:
            t.text2, t.n2 = b.ctypes.data, len(b) - 1
        t.rc_odd_reads = int(bool(rc_odd_reads))
        t.max_reads = int(max_reads) if max_reads is not None else min(0x7FFFFFFF, (len(a) + 3) // 4 + ((len(b) + 3) // 4 if b is not None else 0))
        n = C.c_int(0)
        rc = self.lib.dg_batch_upload_fastq(self.ctx, C.byref(t), C.byref(n))
        self.fastq_need = int(n.value)               # (with DG_ERR_CAPACITY: the reads the texts hold)
        self._chk(rc, "dg_batch_upload_fastq")
        self._n = int(n.value)
        ms = C.c_float(0)
        self.lib.dg_batch_fastq_device_ms(self.ctx, C.byref(ms))
        self.fastq_device_ms = float(ms.value)
        return self._n

    def set_trim(self, adapter=b"", adapter2=None, qual3: int = 0, qual5: int = 0, qual_base: int = 33, min_overlap: int = 3, max_err_permille: int = 100,
                 poly: str = "", poly_min: int = 10, min_len: int = 20, pairs: bool = False, off: bool = False, flags: int | None = None, poly_mask: int | None = None):
        """cut adapters, poly tails and low-quality ends inside every following FASTQ upload of this context (dg_set_trim; the definition is in
        include/dartgpu.h).  adapter2 None: the first adapter; poly: letters of ACGT; off=True: no trimming.  flags / poly_mask: the raw words, for the error tests."""
        if not hasattr(self.lib, "dg_set_trim"):
            raise RuntimeError("this build of libdartgpu.so has no dg_set_trim")
        if off:
            self._chk(self.lib.dg_set_trim(self.ctx, None), "dg_set_trim")
            return
        a = [bytes(adapter), bytes(adapter if adapter2 is None else adapter2)]
        t = Trim()
        t.flags = (TRIM_PAIRS if pairs else 0) if flags is None else flags
        t.qual3, t.qual5, t.qual_base, t.min_overlap, t.max_err_permille = qual3, qual5, qual_base, min_overlap, max_err_permille
        t.poly_mask = sum(1 << "ACGT".index(c) for c in poly.upper()) if poly_mask is None else poly_mask
        t.poly_min, t.min_len = poly_min, min_len
        for i in range(2):
            t.n_adapter[i] = len(a[i])
            C.memmove(t.adapter[i], a[i][:64], min(len(a[i]), 64))
        self._chk(self.lib.dg_set_trim(self.ctx, C.byref(t)), "dg_set_trim")

    def set_umi(self, len1: int = 0, len2: int = 0, skip1: int = 0, skip2: int = 0, sep: bytes = b"_", pairs: bool = False, off: bool = False, flags: int | None = None):
        """cut inline UMIs (the first len bases of a read, then skip bases of linker; slot 1: text 2's reads, or the odd reads of one text with pairs) inside every
        following FASTQ upload of this context and append them to the stored names behind sep (dg_set_umi; the definition is in include/dartgpu.h).  off=True:
        no cut.  flags: the raw word, for the error tests."""
        if off:
            self._chk(self.lib.dg_set_umi(self.ctx, None), "dg_set_umi")
            return
        u = DgUmi()
        u.flags = (1 if pairs else 0) if flags is None else flags
        u.len[0], u.len[1], u.skip[0], u.skip[1] = len1, len2, skip1, skip2
        u.sep = sep if isinstance(sep, bytes) else sep.encode()
        self._chk(self.lib.dg_set_umi(self.ctx, C.byref(u)), "dg_set_umi")

    def trim_stats(self):
        """the last upload's trimming statistics (dg_batch_trim_stats) -> [16] ints; self.trim_device_ms holds the trimming kernels' device time"""
        st = (C.c_uint64 * 16)(); ms = C.c_float(0)
        self._chk(self.lib.dg_batch_trim_stats(self.ctx, st, C.byref(ms)), "dg_batch_trim_stats")
        self.trim_device_ms = float(ms.value)
        return [int(x) for x in st]

    def trim_granules(self):
        """(reads per workgroup of the length kernel, start positions per round of the cutting kernel) (dg_trim_granules)"""
        g = (C.c_int * 2)()
        self._chk(self.lib.dg_trim_granules(g), "dg_trim_granules")
        return int(g[0]), int(g[1])

    def download_reads(self):
        """the batch a FASTQ upload parsed (dg_batch_download_reads) -> (seq_off u32 [n], rlen u16 [n], flat u8, names [n] bytes, stored qualities [n] bytes)"""
        caps = (C.c_size_t * 3)(0, 0, 0); used = (C.c_size_t * 3)()
        n = self._n
        so = np.zeros(max(n, 1), np.uint32); rl = np.zeros(max(n, 1), np.uint16); ho = np.zeros(n + 1, np.uint32); qo = np.zeros(n + 1, np.uint32)
        rc = self.lib.dg_batch_download_reads(self.ctx, so.ctypes.data, rl.ctypes.data, None, ho.ctypes.data, None, qo.ctypes.data, None, caps, used)
        if rc not in (0, -4):
            self._chk(rc, "dg_batch_download_reads")
        flat = np.zeros(max(int(used[0]), 1), np.uint8); hb = np.zeros(max(int(used[1]), 1), np.uint8); qb = np.zeros(max(int(used[2]), 1), np.uint8)
        caps = (C.c_size_t * 3)(int(used[0]), int(used[1]), int(used[2]))
        self._chk(self.lib.dg_batch_download_reads(self.ctx, so.ctypes.data, rl.ctypes.data, flat.ctypes.data, ho.ctypes.data, hb.ctypes.data, qo.ctypes.data, qb.ctypes.data, caps, used),
                  "dg_batch_download_reads")
        hraw, qraw = hb.tobytes(), qb.tobytes()
        names = [hraw[int(ho[k]):int(ho[k + 1])] for k in range(n)]
        quals = [qraw[int(qo[k]):int(qo[k + 1])] for k in range(n)]
        return so[:n], rl[:n], flat[:int(used[0])], names, quals

    def format_sam_resident(self, n_pair_mode: int, unique_only: bool = False):
        """format_sam with the names and qualities a FASTQ upload left in HBM (dg_batch_format_sam_resident) -> (bytes, counters)"""
        nb = C.c_size_t(0); ct = (C.c_uint64 * 3)(); ms = C.c_float(0)
        self._chk(self.lib.dg_batch_format_sam_resident(self.ctx, int(n_pair_mode), SAM_UNIQUE_ONLY if unique_only else 0, C.byref(nb), ct, C.byref(ms)), "dg_batch_format_sam_resident")
        self.sam_device_ms = float(ms.value)
        out = np.zeros(max(int(nb.value), 1), np.uint8)
        self._chk(self.lib.dg_batch_download_sam(self.ctx, out.ctypes.data, int(nb.value)), "dg_batch_download_sam")
        return out[:int(nb.value)].tobytes(), dict(unmapped=int(ct[0]), unique=int(ct[1]), paired=int(ct[2]))

    def device_sam_tensor(self):
        """torch uint8 view of the SAM text in HBM (dg_batch_device_sam), valid until the next upload or run (for RCCL collectives)"""
        import torch
        ptr = C.c_void_p(); nb = C.c_size_t(0)
        self._chk(self.lib.dg_batch_device_sam(self.ctx, C.byref(ptr), C.byref(nb)), "dg_batch_device_sam")
        if not nb.value:
            return torch.empty(0, dtype=torch.uint8, device="cuda")

        class _View:
            pass
        v = _View()
        v.__cuda_array_interface__ = {"shape": (int(nb.value),), "typestr": "|u1", "data": (int(ptr.value), False), "version": 2}
        return torch.as_tensor(v, device="cuda")

    def _bam_result(self, nb, n_raw, ct, ms):
        self.bam_device_ms = float(ms.value)
        split = (C.c_float * 2)()
        self.lib.dg_batch_bam_device_ms(self.ctx, split)
        self.bam_device_ms_split = (float(split[0]), float(split[1]))      # record kernels, BGZF kernels
        self.bam_raw_bytes = int(n_raw.value)
        out = np.zeros(max(int(nb.value), 1), np.uint8)
        self._chk(self.lib.dg_batch_download_bam(self.ctx, out.ctypes.data, int(nb.value)), "dg_batch_download_bam")
        return out[:int(nb.value)].tobytes(), dict(unmapped=int(ct[0]), unique=int(ct[1]), paired=int(ct[2]), records=int(ct[3]), refused=int(ct[4]))

    def format_bam(self, headers, quals, n_pair_mode: int, unique_only: bool = False, raw: bool = False, dynamic: bool = False):
        """BAM of the batch that ran last, made on the device (dg_batch_format_bam + dg_batch_download_bam) -> (bytes, counters): BGZF blocks without the
        file's header and end-of-file block, or with raw=True the uncompressed records; arguments as format_sam; counters: format_sam's three, records
        written and lines refused; self.bam_device_ms holds the kernels' device time, self.bam_raw_bytes the records' size; dynamic=True: BGZF with
        dynamic Huffman codes per strip (DG_BAM_DYNAMIC): a smaller stream of the same records"""
        if not hasattr(self.lib, "dg_batch_format_bam"):
            raise RuntimeError("this build of libdartgpu.so has no dg_batch_format_bam")
        ho, hb = flatten_strings(headers)
        t = SamText()
        t.hdr_off, t.hdr, t.n_pair_mode = ho.ctypes.data, hb.ctypes.data, int(n_pair_mode)
        if quals is not None:
            qo, qb = flatten_strings(quals)
            t.qual_off, t.qual = qo.ctypes.data, qb.ctypes.data
        nb = C.c_size_t(0); n_raw = C.c_size_t(0); ct = (C.c_uint64 * 5)(); ms = C.c_float(0)
        flags = (SAM_UNIQUE_ONLY if unique_only else 0) | (BAM_RAW if raw else 0) | (BAM_DYNAMIC if dynamic else 0)
        self._chk(self.lib.dg_batch_format_bam(self.ctx, C.byref(t), flags, C.byref(nb), C.byref(n_raw), ct, C.byref(ms)), "dg_batch_format_bam")
        return self._bam_result(nb, n_raw, ct, ms)

    def format_bam_resident(self, n_pair_mode: int, unique_only: bool = False, raw: bool = False, dynamic: bool = False):
        """format_bam with the names and qualities a FASTQ upload left in HBM (dg_batch_format_bam_resident) -> (bytes, counters)"""
        nb = C.c_size_t(0); n_raw = C.c_size_t(0); ct = (C.c_uint64 * 5)(); ms = C.c_float(0)
        flags = (SAM_UNIQUE_ONLY if unique_only else 0) | (BAM_RAW if raw else 0) | (BAM_DYNAMIC if dynamic else 0)
        self._chk(self.lib.dg_batch_format_bam_resident(self.ctx, int(n_pair_mode), flags, C.byref(nb), C.byref(n_raw), ct, C.byref(ms)), "dg_batch_format_bam_resident")
        return self._bam_result(nb, n_raw, ct, ms)

    def bgzf_compress(self, data, dynamic: bool = False) -> bytes:
        """any bytes -> BGZF blocks, compressed on the device (dg_bgzf_compress + dg_batch_download_bam); no end-of-file block; self.bam_device_ms holds the
        kernels' device time; dynamic=True: dynamic Huffman codes per strip (dg_bgzf_compress_flags with DG_BGZF_DYNAMIC)"""
        if not hasattr(self.lib, "dg_bgzf_compress"):
            raise RuntimeError("this build of libdartgpu.so has no dg_bgzf_compress")
        a = np.frombuffer(bytes(data) + b"\0", np.uint8)
        nb = C.c_size_t(0); ms = C.c_float(0)
        if dynamic:
            if not hasattr(self.lib, "dg_bgzf_compress_flags"):
                raise RuntimeError("this build of libdartgpu.so has no dg_bgzf_compress_flags")
            self._chk(self.lib.dg_bgzf_compress_flags(self.ctx, a.ctypes.data, len(a) - 1, BGZF_DYNAMIC, C.byref(nb), C.byref(ms)), "dg_bgzf_compress_flags")
        else:
            self._chk(self.lib.dg_bgzf_compress(self.ctx, a.ctypes.data, len(a) - 1, C.byref(nb), C.byref(ms)), "dg_bgzf_compress")
        self.bam_device_ms = float(ms.value)
        out = np.zeros(max(int(nb.value), 1), np.uint8)
        self._chk(self.lib.dg_batch_download_bam(self.ctx, out.ctypes.data, int(nb.value)), "dg_batch_download_bam")
        return out[:int(nb.value)].tobytes()

    def bgzf_granules(self):
        """(strip, segment) of the device's deflate kernel in bytes (dg_bgzf_granules)"""
        g = (C.c_int * 2)()
        self._chk(self.lib.dg_bgzf_granules(g), "dg_bgzf_granules")
        return int(g[0]), int(g[1])

    def bgzf_inflate(self, data) -> bytes:
        """whole BGZF blocks -> their bytes, inflated on the device (dg_bgzf_inflate + dg_inflate_download); self.inflate_device_ms holds the kernel's device
        time, self.inflate_blocks the number of blocks"""
        if not hasattr(self.lib, "dg_bgzf_inflate"):
            raise RuntimeError("this build of libdartgpu.so has no dg_bgzf_inflate")
        a = np.frombuffer(bytes(data) + b"\0", np.uint8)
        nb = C.c_size_t(0); nk = C.c_size_t(0); ms = C.c_float(0)
        self._chk(self.lib.dg_bgzf_inflate(self.ctx, a.ctypes.data, len(a) - 1, C.byref(nb), C.byref(nk), C.byref(ms)), "dg_bgzf_inflate")
        self.inflate_device_ms = float(ms.value); self.inflate_blocks = int(nk.value)
        out = np.zeros(max(int(nb.value), 1), np.uint8)
        self._chk(self.lib.dg_inflate_download(self.ctx, out.ctypes.data, int(nb.value)), "dg_inflate_download")
        return out[:int(nb.value)].tobytes()

    def upload_fastq_bgzf(self, head1, blocks1, head2=None, blocks2=None, rc_odd_reads: bool = False, max_reads: int | None = None, last: bool = False,
                          check_only: bool = False):
        """FASTQ text as head bytes + BGZF blocks per text -> the batch in HBM (dg_batch_upload_fastq_bgzf) -> (n_reads, tail1, tail2, n_unlike): whole records
        only unless last; the tails are what lies behind the last record taken (the next call's heads).  head2 and blocks2 None: one text.  check_only: the
        same counts, no batch.  max_reads None: as many as the texts can hold."""
        if not hasattr(self.lib, "dg_batch_upload_fastq_bgzf"):
            raise RuntimeError("this build of libdartgpu.so has no dg_batch_upload_fastq_bgzf")
        two = head2 is not None or blocks2 is not None
        bufs = [np.frombuffer(bytes(x if x is not None else b"") + b"\0", np.uint8) for x in (head1, blocks1, head2, blocks2)]
        t = FastqBgzf()
        t.head1, t.n_head1, t.blocks1, t.n_blocks1 = bufs[0].ctypes.data, len(bufs[0]) - 1, bufs[1].ctypes.data, len(bufs[1]) - 1
        if two:
            t.head2, t.n_head2, t.blocks2, t.n_blocks2 = bufs[2].ctypes.data, len(bufs[2]) - 1, bufs[3].ctypes.data, len(bufs[3]) - 1
        t.rc_odd_reads, t.last = int(bool(rc_odd_reads)), int(bool(last))
        # (a record has at least four bytes; a block inflates to at most 65536 bytes and is at least 28)
        room = sum(len(bufs[i]) + (len(bufs[i + 1]) // 28 + 1) * 65536 for i in (0, 2))
        t.max_reads = int(max_reads) if max_reads is not None else min(0x7FFFFFFF, room // 4 + 2)
        n = C.c_int(0); tail = (C.c_size_t * 2)(); nu = C.c_uint64(0)
        rc = self.lib.dg_batch_upload_fastq_bgzf(self.ctx, C.byref(t), FQ_CHECK_ONLY if check_only else 0, C.byref(n), tail, C.byref(nu))
        self.fastq_need = int(n.value)
        self._chk(rc, "dg_batch_upload_fastq_bgzf")
        self._n = 0 if check_only else int(n.value)
        ms = C.c_float(0)
        self.lib.dg_batch_fastq_device_ms(self.ctx, C.byref(ms))
        self.fastq_device_ms = float(ms.value)
        t1 = np.zeros(max(int(tail[0]), 1), np.uint8); t2 = np.zeros(max(int(tail[1]), 1), np.uint8)
        self._chk(self.lib.dg_batch_download_fastq_tail(self.ctx, t1.ctypes.data, int(tail[0]), t2.ctypes.data, int(tail[1])), "dg_batch_download_fastq_tail")
        return int(n.value), t1[:int(tail[0])].tobytes(), (t2[:int(tail[1])].tobytes() if two else None), int(nu.value)

    def inflate_granules(self):
        """(blocks per workgroup, tokens decoded per write-out round) of the device's inflate kernel (dg_inflate_granules)"""
        if not hasattr(self.lib, "dg_inflate_granules"):
            raise RuntimeError("this build of libdartgpu.so has no dg_inflate_granules")
        g = (C.c_int * 2)()
        self._chk(self.lib.dg_inflate_granules(g), "dg_inflate_granules")
        return int(g[0]), int(g[1])

    def device_bam_tensor(self):
        """torch uint8 view of the BAM bytes in HBM (dg_batch_device_bam), valid until the next upload or run"""
        import torch
        ptr = C.c_void_p(); nb = C.c_size_t(0)
        self._chk(self.lib.dg_batch_device_bam(self.ctx, C.byref(ptr), C.byref(nb)), "dg_batch_device_bam")
        if not nb.value:
            return torch.empty(0, dtype=torch.uint8, device="cuda")

        class _View:
            pass
        v = _View()
        v.__cuda_array_interface__ = {"shape": (int(nb.value),), "typestr": "|u1", "data": (int(ptr.value), False), "version": 2}
        return torch.as_tensor(v, device="cuda")

    # ---- the splice-junction table on the device (dg_sj_*): counted per batch, sorted and printed at the end of the job ----
    def sj_granules(self):
        """(tuples one workgroup of the insert kernel takes, the smallest table in slots) (dg_sj_granules)"""
        g = (C.c_int * 2)()
        self._chk(self.lib.dg_sj_granules(g), "dg_sj_granules")
        return int(g[0]), int(g[1])

    def sj_reserve(self, slots: int):
        self._chk(self.lib.dg_sj_reserve(self.ctx, int(slots)), "dg_sj_reserve")

    def sj_reset(self):
        self._chk(self.lib.dg_sj_reset(self.ctx), "dg_sj_reset")

    def accumulate_sj(self) -> int:
        """counts the junction tuples of the batch that ran last in the context's table (dg_batch_accumulate_sj) -> the number of tuples"""
        n = C.c_size_t(0)
        self._chk(self.lib.dg_batch_accumulate_sj(self.ctx, C.byref(n)), "dg_batch_accumulate_sj")
        return int(n.value)

    def sj_add(self, entries):
        """counts host entries with their counts (dg_sj_add): an SJ_ENTRY array, or any sequence of (g1, g2, count)"""
        if isinstance(entries, np.ndarray) and entries.dtype == SJ_ENTRY:
            a = np.ascontiguousarray(entries)
        else:
            rows = list(entries)
            a = np.zeros(len(rows), SJ_ENTRY)
            for k, t in enumerate(rows):
                a[k]["g1"], a[k]["g2"], a[k]["count"] = int(t[0]), int(t[1]), int(t[2]) if len(t) > 2 else 1
        keep = a if len(a) else np.zeros(1, SJ_ENTRY)
        self._chk(self.lib.dg_sj_add(self.ctx, keep.ctypes.data, len(a)), "dg_sj_add")

    def sj_merge(self, src: "DartGPU"):
        """folds src's table into this context's and leaves src's empty (dg_sj_merge)"""
        self._chk(self.lib.dg_sj_merge(self.ctx, src.ctx), "dg_sj_merge")

    def sj_finish(self, entries_only: bool = False):
        """the table sorted, mapped to chromosomes and printed on the device (dg_sj_finish + dg_sj_download) -> (SJ_ENTRY array, the bytes of
        junctions.tab); self.sj_lines = the reference's "# of splice junctions", self.sj_device_ms = the kernels' device time"""
        ne = C.c_size_t(0); nl = C.c_size_t(0); nb = C.c_size_t(0); ms = C.c_float(0)
        self._chk(self.lib.dg_sj_finish(self.ctx, SJ_ENTRIES_ONLY if entries_only else 0, C.byref(ne), C.byref(nl), C.byref(nb), C.byref(ms)), "dg_sj_finish")
        self.sj_lines, self.sj_device_ms = int(nl.value), float(ms.value)
        ent = np.zeros(max(int(ne.value), 1), SJ_ENTRY); text = np.zeros(max(int(nb.value), 1), np.uint8)
        self._chk(self.lib.dg_sj_download(self.ctx, ent.ctypes.data, int(ne.value), text.ctypes.data, int(nb.value)), "dg_sj_download")
        return ent[:int(ne.value)], text[:int(nb.value)].tobytes()

    # ---- gene-level read counts on the device (dg_gene_*): counted per batch from the records in HBM, merged at the end of the job ----
    def gene_granules(self):
        """(units per workgroup of the counting kernel, the wave width its combining uses) (dg_gene_granules)"""
        g = (C.c_int * 2)()
        self._chk(self.lib.dg_gene_granules(g), "dg_gene_granules")
        return int(g[0]), int(g[1])

    def gene_set_annotation(self, n_genes: int, exons) -> int:
        """flattens and uploads the annotation, kept with the index and shared by clones (dg_gene_set_annotation) -> the number of segments;
        exons: a GENE_EXON array, or any sequence of (chr, start, end, strand, gene) with 0-based half-open coordinates"""
        if isinstance(exons, np.ndarray) and exons.dtype == GENE_EXON:
            a = np.ascontiguousarray(exons)
        else:
            rows = list(exons)
            a = np.zeros(len(rows), GENE_EXON)
            for k, t in enumerate(rows):
                a[k] = tuple(int(x) for x in t)
        keep = a if len(a) else np.zeros(1, GENE_EXON)
        ann = GeneAnnot(int(n_genes), 0, len(a), keep.ctypes.data)
        n = C.c_size_t(0)
        self._chk(self.lib.dg_gene_set_annotation(self.ctx, C.byref(ann), C.byref(n)), "dg_gene_set_annotation")
        self.gene_rows = 4 + int(n_genes)
        return int(n.value)

    def accumulate_genes(self, n_pair_mode: int, min_mapq: int = 4) -> int:
        """counts the units of the batch that ran last in the context's table (dg_batch_accumulate_genes) -> the number of units"""
        n = C.c_size_t(0)
        self._chk(self.lib.dg_batch_accumulate_genes(self.ctx, int(n_pair_mode), int(min_mapq), C.byref(n)), "dg_batch_accumulate_genes")
        return int(n.value)

    def gene_count_records(self, reads, reports, cigar, n_pair_mode: int, min_mapq: int = 4) -> int:
        """counts host records (READ_OUT, REPORT_OUT, CIGAR words) through the same kernel (dg_gene_count_records) -> the number of units"""
        rd = np.ascontiguousarray(reads, READ_OUT); rp = np.ascontiguousarray(reports, REPORT_OUT); cg = np.ascontiguousarray(cigar, np.uint32)
        n = C.c_size_t(0)
        self._chk(self.lib.dg_gene_count_records(self.ctx, len(rd), int(n_pair_mode), int(min_mapq), rd.ctypes.data if len(rd) else None, rp.ctypes.data if len(rp) else None, len(rp),
                                                 cg.ctypes.data if len(cg) else None, len(cg), C.byref(n)), "dg_gene_count_records")
        return int(n.value)

    def gene_add(self, counts):
        """host counts folded in (dg_gene_add): uint64 [4 + n_genes, 3]"""
        a = np.ascontiguousarray(counts, np.uint64)
        self._chk(self.lib.dg_gene_add(self.ctx, a.ctypes.data, a.shape[0]), "dg_gene_add")

    def gene_merge(self, src: "DartGPU"):
        """adds src's table to this context's and leaves src's empty (dg_gene_merge)"""
        self._chk(self.lib.dg_gene_merge(self.ctx, src.ctx), "dg_gene_merge")

    def gene_reset(self):
        self._chk(self.lib.dg_gene_reset(self.ctx), "dg_gene_reset")

    def gene_counts(self, n_rows: int | None = None) -> np.ndarray:
        """the context's table (dg_gene_download) -> uint64 [4 + n_genes, 3]; n_rows: of a table counted under an annotation this object did not set (a clone's)"""
        rows = int(n_rows if n_rows is not None else getattr(self, "gene_rows", None) or self._parent.gene_rows)
        out = np.zeros((rows, 3), np.uint64)
        self._chk(self.lib.dg_gene_download(self.ctx, out.ctypes.data, rows), "dg_gene_download")
        ms = C.c_float(0)
        self._chk(self.lib.dg_gene_device_ms(self.ctx, C.byref(ms)), "dg_gene_device_ms")
        self.gene_device_ms = float(ms.value)
        return out

    # ---- coordinate-sorted BAM on the device (dg_bam_sort_*): every batch's records stay in HBM, one sort at the end of the job ----
    def bam_sort_granules(self):
        """(reads per workgroup of the two key kernels, pairs per tile of the sorter, the store's smallest size in bytes) (dg_bam_sort_granules)"""
        g = (C.c_int * 3)()
        self._chk(self.lib.dg_bam_sort_granules(g), "dg_bam_sort_granules")
        return int(g[0]), int(g[1]), int(g[2])

    def bam_sort_info(self):
        """the store: dict(records, bytes, segments, growths = the calls in which it grew) (dg_bam_sort_info, a test hook)"""
        o = (C.c_size_t * 4)()
        self._chk(self.lib.dg_bam_sort_info(self.ctx, o), "dg_bam_sort_info")
        return dict(records=int(o[0]), bytes=int(o[1]), segments=int(o[2]), growths=int(o[3]))

    def accumulate_bam(self, ordinal: int) -> int:
        """appends the uncompressed records the last format_bam left for the current batch to the context's store under this ordinal
        (dg_batch_accumulate_bam) -> the number of records; self.bam_sort_added_bytes holds their bytes"""
        n = C.c_size_t(0); nb = C.c_size_t(0)
        self._chk(self.lib.dg_batch_accumulate_bam(self.ctx, int(ordinal), C.byref(n), C.byref(nb)), "dg_batch_accumulate_bam")
        self.bam_sort_added_bytes = int(nb.value)
        split = (C.c_float * 5)()
        self.lib.dg_bam_sort_device_ms(self.ctx, split, None)
        self.bam_sort_accumulate_ms = float(split[4])        # device time of the key kernels and the copy
        return int(n.value)

    def bam_sort_add(self, data, ordinal: int) -> int:
        """appends whole uncompressed BAM records from host memory (dg_bam_sort_add) -> the number of records"""
        a = np.frombuffer(bytes(data) + b"\0", np.uint8)
        n = C.c_size_t(0)
        self._chk(self.lib.dg_bam_sort_add(self.ctx, a.ctypes.data, len(a) - 1, int(ordinal), C.byref(n)), "dg_bam_sort_add")
        return int(n.value)

    def bam_sort_merge(self, src: "DartGPU"):
        """appends src's store to this context's and leaves src's empty (dg_bam_sort_merge)"""
        self._chk(self.lib.dg_bam_sort_merge(self.ctx, src.ctx), "dg_bam_sort_merge")

    def bam_sort_reset(self):
        self._chk(self.lib.dg_bam_sort_reset(self.ctx), "dg_bam_sort_reset")

    def bam_sort_finish(self):
        """sorts the store's records into one contiguous array in HBM (dg_bam_sort_finish) -> (records, raw bytes); self.bam_sort_device_ms holds the
        device time, self.bam_sort_device_ms_split (segment ordering, sort, lengths + scan, gather), self.bam_sort_passes the sorter's passes"""
        n = C.c_size_t(0); nb = C.c_size_t(0); ms = C.c_float(0)
        self._chk(self.lib.dg_bam_sort_finish(self.ctx, C.byref(n), C.byref(nb), C.byref(ms)), "dg_bam_sort_finish")
        split = (C.c_float * 5)(); passes = C.c_int(0)
        self.lib.dg_bam_sort_device_ms(self.ctx, split, C.byref(passes))
        self.bam_sort_device_ms, self.bam_sort_device_ms_split, self.bam_sort_passes = float(ms.value), tuple(float(x) for x in split[:4]), int(passes.value)
        return int(n.value), int(nb.value)

    def bam_sort_compress(self, off: int, length: int, raw: bool = False, dynamic: bool = False) -> bytes:
        """one range of the sorted array as BGZF blocks, or with raw=True as it is (dg_bam_sort_compress + dg_batch_download_bam); off must be a multiple
        of 0xff00, length such a multiple or reach the array's end; self.bam_device_ms holds the BGZF kernels' device time"""
        nb = C.c_size_t(0); ms = C.c_float(0)
        flags = BAM_RAW if raw else (BGZF_DYNAMIC if dynamic else 0)
        self._chk(self.lib.dg_bam_sort_compress(self.ctx, int(off), int(length), flags, C.byref(nb), C.byref(ms)), "dg_bam_sort_compress")
        self.bam_device_ms = float(ms.value)
        out = np.zeros(max(int(nb.value), 1), np.uint8)
        self._chk(self.lib.dg_batch_download_bam(self.ctx, out.ctypes.data, int(nb.value)), "dg_batch_download_bam")
        return out[:int(nb.value)].tobytes()

    # ---- the BAM index of the sorted array (dg_bam_index_*): the .bai, built in HBM behind bam_sort_finish ----
    def bam_index_granules(self):
        """(records per workgroup of the per-record kernel, chunks per tile of the sorter) (dg_bam_index_granules)"""
        g = (C.c_int * 2)()
        self._chk(self.lib.dg_bam_index_granules(g), "dg_bam_index_granules")
        return int(g[0]), int(g[1])

    def bam_index_finish(self, first_block_offset: int, block_sizes=None) -> bytes:
        """the .bai of the sorted array (dg_bam_index_finish + dg_bam_index_download); block_sizes=None: the compressed sizes the last bam_sort_compress of
        every block left, else one size per block of 0xff00 raw bytes.  self.bam_index_stats = (placed records, n_no_coor, bins, chunks before the merge,
        chunks after it, linear-index entries), self.bam_index_device_ms = the kernels' device time"""
        nb = C.c_size_t(0); ms = C.c_float(0); st = (C.c_uint64 * 6)()
        sizes, n = None, 0
        if block_sizes is not None:
            sizes = np.ascontiguousarray(np.asarray(block_sizes, np.uint32).reshape(-1)); n = len(sizes)
            sizes = np.concatenate([sizes, np.zeros(1, np.uint32)])          # (never an empty buffer)
        self._chk(self.lib.dg_bam_index_finish(self.ctx, int(first_block_offset), sizes.ctypes.data if sizes is not None else None, n, C.byref(nb), st, C.byref(ms)),
                  "dg_bam_index_finish")
        self.bam_index_stats, self.bam_index_device_ms = tuple(int(x) for x in st), float(ms.value)
        out = np.zeros(max(int(nb.value), 1), np.uint8)
        self._chk(self.lib.dg_bam_index_download(self.ctx, out.ctypes.data, int(nb.value)), "dg_bam_index_download")
        return out[:int(nb.value)].tobytes()

    # ---- the coverage track of the sorted array (dg_bam_coverage_*): the bedGraph, built in HBM behind bam_sort_finish ----
    def bam_coverage_granules(self):
        """(records / events / entries per workgroup, events per tile of the sorter) (dg_bam_coverage_granules)"""
        g = (C.c_int * 2)()
        self._chk(self.lib.dg_bam_coverage_granules(g), "dg_bam_coverage_granules")
        return int(g[0]), int(g[1])

    def bam_coverage_finish(self, exclude: int = 0x704, min_mapq: int = 0, strand=None, entries_only: bool = False):
        """the coverage track of the sorted array (dg_bam_coverage_finish + dg_bam_coverage_download) -> (COV_ENTRY array, the bedGraph's bytes); strand: None,
        "+" or "-" (a second mate counts for the opposite strand).  self.bam_coverage_stats = (records counted, blocks, breakpoints, entries, covered bases,
        aligned bases, largest depth), self.bam_coverage_device_ms = the kernels' device time, self.bam_coverage_device_ms_split = (counting walk, emitting
        walk, event sort, scans and compaction, entries and text), self.bam_coverage_passes = the sorter's passes"""
        flags = (COV_ENTRIES_ONLY if entries_only else 0) | {None: 0, "+": COV_STRAND_PLUS, "-": COV_STRAND_MINUS}[strand]
        ne = C.c_size_t(0); nb = C.c_size_t(0); ms = C.c_float(0); st = (C.c_uint64 * 7)()
        self._chk(self.lib.dg_bam_coverage_finish(self.ctx, flags, int(exclude), int(min_mapq), C.byref(ne), C.byref(nb), st, C.byref(ms)), "dg_bam_coverage_finish")
        self.bam_coverage_stats, self.bam_coverage_device_ms = tuple(int(x) for x in st), float(ms.value)
        split = (C.c_float * 5)(); passes = C.c_int(0)
        self._chk(self.lib.dg_bam_coverage_device_ms(self.ctx, split, C.byref(passes)), "dg_bam_coverage_device_ms")
        self.bam_coverage_device_ms_split, self.bam_coverage_passes = tuple(float(x) for x in split), int(passes.value)
        ent = np.zeros(max(int(ne.value), 1), COV_ENTRY); text = np.zeros(max(int(nb.value), 1), np.uint8)
        self._chk(self.lib.dg_bam_coverage_download(self.ctx, ent.ctypes.data, int(ne.value), text.ctypes.data, int(nb.value)), "dg_bam_coverage_download")
        return ent[:int(ne.value)], text[:int(nb.value)].tobytes()

    # ---- the allele counts of the sorted array (dg_bam_pileup_*): the variant-site table, built in HBM behind bam_sort_finish ----
    def bam_pileup_granules(self):
        """(records / events / sites per workgroup, events per tile of the sorter, reference bases per packed compare step) (dg_bam_pileup_granules)"""
        g = (C.c_int * 3)()
        self._chk(self.lib.dg_bam_pileup_granules(g), "dg_bam_pileup_granules")
        return int(g[0]), int(g[1]), int(g[2])

    def bam_pileup_finish(self, exclude: int = 0x704, min_mapq: int = 0, min_alt: int = 2, entries_only: bool = False):
        """the allele counts of the sorted array (dg_bam_pileup_finish + dg_bam_pileup_download) -> (SITE_ENTRY array, the table's bytes).
        self.bam_pileup_stats = (records counted, blocks, aligned bases, mismatching bases, deleted bases, insertions, sites before the min_alt filter, sites kept,
        records left out, largest depth at a kept site), self.bam_pileup_device_ms = the kernels' device time, self.bam_pileup_device_ms_split = (counting walk,
        emitting walk, event sort, scans and compaction, sites and text), self.bam_pileup_passes = the sorter's passes"""
        ne = C.c_size_t(0); nb = C.c_size_t(0); ms = C.c_float(0); st = (C.c_uint64 * 10)()
        self._chk(self.lib.dg_bam_pileup_finish(self.ctx, PU_ENTRIES_ONLY if entries_only else 0, int(exclude), int(min_mapq), int(min_alt), C.byref(ne), C.byref(nb), st, C.byref(ms)),
                  "dg_bam_pileup_finish")
        self.bam_pileup_stats, self.bam_pileup_device_ms = tuple(int(x) for x in st), float(ms.value)
        split = (C.c_float * 5)(); passes = C.c_int(0)
        self._chk(self.lib.dg_bam_pileup_device_ms(self.ctx, split, C.byref(passes)), "dg_bam_pileup_device_ms")
        self.bam_pileup_device_ms_split, self.bam_pileup_passes = tuple(float(x) for x in split), int(passes.value)
        ent = np.zeros(max(int(ne.value), 1), SITE_ENTRY); text = np.zeros(max(int(nb.value), 1), np.uint8)
        self._chk(self.lib.dg_bam_pileup_download(self.ctx, ent.ctypes.data, int(ne.value), text.ctypes.data, int(nb.value)), "dg_bam_pileup_download")
        return ent[:int(ne.value)], text[:int(nb.value)].tobytes()

    # ---- the QC tables of the sorted array (dg_bam_qc_*): flag summary, histograms and per-cycle tables, built in HBM behind bam_sort_finish ----
    def bam_qc_granules(self):
        """(threads per workgroup, bases per lane, bases per step of the lanes that share a record, trips between two flushes, the record length above which per-base terms go straight
        to the global words) (dg_bam_qc_granules)"""
        g = (C.c_int * 5)()
        self._chk(self.lib.dg_bam_qc_granules(g), "dg_bam_qc_granules")
        return tuple(int(x) for x in g)

    def bam_qc_finish(self, exclude: int = 0x904, min_mapq: int = 0):
        """the QC tables of the sorted array (dg_bam_qc_finish + dg_bam_qc_download) -> dict of numpy views into one uint64 array: "words" (all of them), "FS"
        [2, 16], "CH" [n_chr + 1, 2], "MQ" [256], "IS" [3, 8001], "RL" [2, 512], "PC" [2, 12, 512], "ID" [2, 65], "SN" [32].  self.bam_qc_device_ms = the
        kernels' device time, self.bam_qc_device_ms_split = (per-record tables, per-cycle pass)"""
        nw = C.c_size_t(0); ms = C.c_float(0)
        self._chk(self.lib.dg_bam_qc_finish(self.ctx, 0, int(exclude), int(min_mapq), C.byref(nw), C.byref(ms)), "dg_bam_qc_finish")
        self.bam_qc_device_ms = float(ms.value)
        split = (C.c_float * 2)()
        self._chk(self.lib.dg_bam_qc_device_ms(self.ctx, split), "dg_bam_qc_device_ms")
        self.bam_qc_device_ms_split = tuple(float(x) for x in split)
        words = np.zeros(int(nw.value), np.uint64)
        self._chk(self.lib.dg_bam_qc_download(self.ctx, words.ctypes.data, len(words)), "dg_bam_qc_download")
        return qc_views(self.lib, words, len(self.index.names))

    # ---- transcript-level expression on the device (dg_tx_*): equivalence classes per batch in a table in HBM, an EM over them at the end of the job ----
    def tx_granules(self):
        """(units per workgroup of the compatibility passes, the wave width) (dg_tx_granules)"""
        g = (C.c_int * 2)()
        self._chk(self.lib.dg_tx_granules(g), "dg_tx_granules")
        return int(g[0]), int(g[1])

    def tx_set_annotation(self, tx, exons):
        """flattens and uploads the transcript annotation, kept with the index and shared by clones (dg_tx_set_annotation) -> (merged exons, segments);
        tx: an RNA_TX array, exons: an RNA_EXON array, 0-based half-open coordinates"""
        t = np.ascontiguousarray(tx, RNA_TX); e = np.ascontiguousarray(exons, RNA_EXON)
        keep_t = t if len(t) else np.zeros(1, RNA_TX); keep_e = e if len(e) else np.zeros(1, RNA_EXON)
        ann = RnaAnnot(len(t), 0, len(e), keep_t.ctypes.data, keep_e.ctypes.data)
        nm, ns = C.c_size_t(0), C.c_size_t(0)
        self._chk(self.lib.dg_tx_set_annotation(self.ctx, C.byref(ann), C.byref(nm), C.byref(ns)), "dg_tx_set_annotation")
        return int(nm.value), int(ns.value)

    def accumulate_tx(self, n_pair_mode: int, min_mapq: int = 4, strand_mode: int = 0) -> int:
        """folds the units of the batch that ran last into the context's class table (dg_batch_accumulate_tx) -> the number of units"""
        n = C.c_size_t(0)
        self._chk(self.lib.dg_batch_accumulate_tx(self.ctx, int(n_pair_mode), int(min_mapq), int(strand_mode), C.byref(n)), "dg_batch_accumulate_tx")
        return int(n.value)

    def tx_count_records(self, reads, reports, cigar, n_pair_mode: int, min_mapq: int = 4, strand_mode: int = 0) -> int:
        """host records (READ_OUT, REPORT_OUT, CIGAR words) through the same kernels (dg_tx_count_records) -> the number of units"""
        rd = np.ascontiguousarray(reads, READ_OUT); rp = np.ascontiguousarray(reports, REPORT_OUT); cg = np.ascontiguousarray(cigar, np.uint32)
        n = C.c_size_t(0)
        self._chk(self.lib.dg_tx_count_records(self.ctx, len(rd), int(n_pair_mode), int(min_mapq), int(strand_mode), rd.ctypes.data if len(rd) else None,
                                               rp.ctypes.data if len(rp) else None, len(rp), cg.ctypes.data if len(cg) else None, len(cg), C.byref(n)), "dg_tx_count_records")
        return int(n.value)

    def tx_merge(self, src: "DartGPU"):
        """folds src's class table into this context's and leaves src's empty (dg_tx_merge)"""
        self._chk(self.lib.dg_tx_merge(self.ctx, src.ctx), "dg_tx_merge")

    def tx_add(self, off, ids, count, words8):
        """a downloaded class table folded in (dg_tx_add): uint64 off [n + 1], uint32 ids, uint64 count [n], uint64 words [8]"""
        o = np.ascontiguousarray(off, np.uint64); i = np.ascontiguousarray(ids, np.uint32); k = np.ascontiguousarray(count, np.uint64); w = np.ascontiguousarray(words8, np.uint64)
        assert len(w) == 8 and (len(k) == 0 or len(o) == len(k) + 1)
        self._chk(self.lib.dg_tx_add(self.ctx, o.ctypes.data if len(k) else None, i.ctypes.data if len(i) else None, k.ctypes.data if len(k) else None, len(k), w.ctypes.data), "dg_tx_add")

    def tx_reset(self):
        self._chk(self.lib.dg_tx_reset(self.ctx), "dg_tx_reset")

    def tx_classes(self):
        """the context's class table (dg_tx_classes_size + dg_tx_classes_download) -> (off uint64 [n + 1], ids uint32, count uint64 [n], words uint64 [8])"""
        nc, nm = C.c_size_t(0), C.c_size_t(0)
        self._chk(self.lib.dg_tx_classes_size(self.ctx, C.byref(nc), C.byref(nm)), "dg_tx_classes_size")
        off = np.zeros(nc.value + 1, np.uint64); ids = np.zeros(max(nm.value, 1), np.uint32); cnt = np.zeros(max(nc.value, 1), np.uint64); words = np.zeros(8, np.uint64)
        self._chk(self.lib.dg_tx_classes_download(self.ctx, off.ctypes.data, ids.ctypes.data, cnt.ctypes.data, nc.value, nm.value, words.ctypes.data), "dg_tx_classes_download")
        split = (C.c_float * 3)()
        self._chk(self.lib.dg_tx_device_ms(self.ctx, split), "dg_tx_device_ms")
        self.tx_device_ms_split = tuple(float(x) for x in split)
        return off, ids[:nm.value], cnt[:nc.value], words

    def tx_finish(self, frag_mean: int = 200, max_rounds: int = 1000) -> np.ndarray:
        """the EM over the context's class table (dg_tx_finish + dg_tx_download) -> uint64 [n_tx + 16]: S and the 16 summary words; self.tx_em_device_ms =
        its device time"""
        nw, ms = C.c_size_t(0), C.c_float(0)
        self._chk(self.lib.dg_tx_finish(self.ctx, 0, int(frag_mean), int(max_rounds), C.byref(nw), C.byref(ms)), "dg_tx_finish")
        self.tx_em_device_ms = float(ms.value)
        words = np.zeros(int(nw.value), np.uint64)
        self._chk(self.lib.dg_tx_download(self.ctx, words.ctypes.data, len(words)), "dg_tx_download")
        return words

    def tx_text(self, words, tx, exons, names) -> bytes:
        """the text of result words (dg_tx_format, on the host)"""
        return tx_text(self.lib, words, tx, exons, names)

    # ---- the RNA-seq metrics of the sorted array (dg_rna_set_annotation, dg_bam_rna_*): base classes, strand and gene-body coverage, built in HBM ----
    def rna_set_annotation(self, tx, exons):
        """flattens and uploads the transcript annotation, kept with the index and shared by clones (dg_rna_set_annotation) -> (segments, eligible
        transcripts); tx: an RNA_TX array, exons: an RNA_EXON array, 0-based half-open coordinates"""
        t = np.ascontiguousarray(tx, RNA_TX); e = np.ascontiguousarray(exons, RNA_EXON)
        keep_t = t if len(t) else np.zeros(1, RNA_TX); keep_e = e if len(e) else np.zeros(1, RNA_EXON)
        ann = RnaAnnot(len(t), 0, len(e), keep_t.ctypes.data, keep_e.ctypes.data)
        ns, ne = C.c_size_t(0), C.c_size_t(0)
        self._chk(self.lib.dg_rna_set_annotation(self.ctx, C.byref(ann), C.byref(ns), C.byref(ne)), "dg_rna_set_annotation")
        return int(ns.value), int(ne.value)

    def bam_rna_granules(self):
        """(records per workgroup trip of the class pass, transcripts per workgroup trip of the body pass) (dg_bam_rna_granules)"""
        g = (C.c_int * 2)()
        self._chk(self.lib.dg_bam_rna_granules(g), "dg_bam_rna_granules")
        return int(g[0]), int(g[1])

    def bam_rna_finish(self, exclude: int = 0x904, min_mapq: int = 0, min_cov: int = 100):
        """the RNA-seq metrics of the sorted array (dg_bam_rna_finish + dg_bam_rna_download) -> dict of numpy views into one uint64 array: "words" (all of
        them), "BA" [5], "RC" [5], "ST" [4], "BC" [3, 100], "SN" [16].  self.bam_rna_device_ms = the kernels' device time, self.bam_rna_device_ms_split =
        (class pass, events and sort, body pass)"""
        nw, ms = C.c_size_t(0), C.c_float(0)
        self._chk(self.lib.dg_bam_rna_finish(self.ctx, 0, int(exclude), int(min_mapq), int(min_cov), C.byref(nw), C.byref(ms)), "dg_bam_rna_finish")
        self.bam_rna_device_ms = float(ms.value)
        split = (C.c_float * 3)()
        self._chk(self.lib.dg_bam_rna_device_ms(self.ctx, split), "dg_bam_rna_device_ms")
        self.bam_rna_device_ms_split = tuple(float(x) for x in split)
        words = np.zeros(int(nw.value), np.uint64)
        self._chk(self.lib.dg_bam_rna_download(self.ctx, words.ctypes.data, len(words)), "dg_bam_rna_download")
        return rna_views(self.lib, words)

    def bam_rna_text(self, words) -> bytes:
        """the text of RNA-metrics words (a dict of bam_rna_finish, or the flat array) (dg_bam_rna_format, on the host)"""
        return rna_text(self.lib, words)

    def bam_qc_text(self, words) -> bytes:
        """the text of QC words (a dict of bam_qc_finish, or the flat array) with the index's chromosome names and lengths (dg_bam_qc_format, on the host)"""
        w = words["words"] if isinstance(words, dict) else words
        return qc_text(self.lib, w, self.index.names, self.index.chr_len)

    # ---- duplicate marking of the sorted array (dg_bam_markdup_*): flag 0x400 written in HBM behind bam_sort_finish, before bam_sort_compress ----
    def bam_markdup_granules(self):
        """(records / candidates / pairs / ends per workgroup, items per tile of the sorter, the largest run of equal name hashes that is not crowded)
        (dg_bam_markdup_granules)"""
        g = (C.c_int * 3)()
        self._chk(self.lib.dg_bam_markdup_granules(g), "dg_bam_markdup_granules")
        return int(g[0]), int(g[1]), int(g[2])

    def bam_markdup_finish(self, count_only: bool = False):
        """marks the duplicates of the sorted array in place (dg_bam_markdup_finish; count_only: decides and counts, writes no flag) -> the stats, also kept as
        self.bam_markdup_stats = (examined records, pairs, fragments, duplicate pairs, duplicate fragments, candidates in crowded runs, records that leave
        with 0x400, the largest family); self.bam_markdup_device_ms = the kernels' device time, self.bam_markdup_device_ms_split = (record pass, mate sort and
        search, pair sorts, end sorts, family scan and flag writes, counting and emitting), self.bam_markdup_passes = the sorter's passes"""
        ms = C.c_float(0); st = (C.c_uint64 * 8)()
        self._chk(self.lib.dg_bam_markdup_finish(self.ctx, MD_COUNT_ONLY if count_only else 0, st, C.byref(ms)), "dg_bam_markdup_finish")
        self.bam_markdup_stats, self.bam_markdup_device_ms = tuple(int(x) for x in st), float(ms.value)
        split = (C.c_float * 6)(); passes = C.c_int(0)
        self._chk(self.lib.dg_bam_markdup_device_ms(self.ctx, split, C.byref(passes)), "dg_bam_markdup_device_ms")
        self.bam_markdup_device_ms_split, self.bam_markdup_passes = tuple(float(x) for x in split), int(passes.value)
        return self.bam_markdup_stats

    # ---- UMI-aware duplicate marking of the sorted array (dg_bam_markdup_umi_*): bam_markdup_finish with the UMI at the end of the name in the signature ----
    def bam_markdup_umi_granules(self):
        """bam_markdup_granules and the largest family (groups of one position) that is clustered (dg_bam_markdup_umi_granules)"""
        g = (C.c_int * 4)()
        self._chk(self.lib.dg_bam_markdup_umi_granules(g), "dg_bam_markdup_umi_granules")
        return tuple(int(x) for x in g)

    def bam_markdup_umi_finish(self, max_edit: int = 0, sep: bytes = b"_", count_only: bool = False):
        """marks the duplicates of the sorted array in place with the UMI behind the last `sep` of a name as part of the signature (dg_bam_markdup_umi_finish;
        max_edit 1: UMIs one letter apart are clustered; count_only: decides and counts, writes no flag) -> the stats, also kept as self.bam_markdup_umi_stats =
        bam_markdup_stats' first seven, the largest cluster, examined records with a UMI, pair families of several groups, absorbed groups, crowded families;
        self.bam_markdup_umi_device_ms = the kernels' device time, self.bam_markdup_umi_device_ms_split = (record pass, mate sort and search, pair sorts, end
        sorts, heads groups and families, clustering, flag writes, counting and emitting), self.bam_markdup_umi_passes = the sorter's passes"""
        sep = sep.encode() if isinstance(sep, str) else bytes(sep)
        if len(sep) != 1:
            raise ValueError("sep is one byte")
        rules = DgUmiRules(0, int(max_edit), sep, b"")
        ms = C.c_float(0); st = (C.c_uint64 * 12)()
        self._chk(self.lib.dg_bam_markdup_umi_finish(self.ctx, C.byref(rules), MD_COUNT_ONLY if count_only else 0, st, C.byref(ms)), "dg_bam_markdup_umi_finish")
        self.bam_markdup_umi_stats, self.bam_markdup_umi_device_ms = tuple(int(x) for x in st), float(ms.value)
        split = (C.c_float * 8)(); passes = C.c_int(0)
        self._chk(self.lib.dg_bam_markdup_umi_device_ms(self.ctx, split, C.byref(passes)), "dg_bam_markdup_umi_device_ms")
        self.bam_markdup_umi_device_ms_split, self.bam_markdup_umi_passes = tuple(float(x) for x in split), int(passes.value)
        return self.bam_markdup_umi_stats

    # ---- MD / NM / ts on the sorted array (dg_bam_tags_*): behind bam_sort_finish (and bam_markdup_finish), before bam_sort_compress ----
    def bam_tags_granules(self):
        """(records per workgroup of the length pass, lanes per record of the write pass's copy, bases per compare step) (dg_bam_tags_granules)"""
        g = (C.c_int * 3)()
        self._chk(self.lib.dg_bam_tags_granules(g), "dg_bam_tags_granules")
        return int(g[0]), int(g[1]), int(g[2])

    def bam_tags_finish(self, md: bool = True, nm: bool = True, ts: bool = True, flags=None):
        """rewrites the sorted array with MD:Z, NM (edit distance) and ts:A (dg_bam_tags_finish; flags: the DG_TAG_* bits instead of the three switches) ->
        (raw bytes of the new array, stats); the stats, also kept as self.bam_tags_stats = (records rewritten, copied verbatim: not eligible, copied verbatim:
        aux unreadable, old tags removed, mismatches, inserted + deleted bases, ts written, introns without ts: no motif | conflict << 32);
        self.bam_tags_device_ms = the kernels' device time, self.bam_tags_device_ms_split = (length pass, write pass)"""
        if flags is None:
            flags = (TAG_MD if md else 0) | (TAG_NM if nm else 0) | (TAG_TS if ts else 0)
        nb = C.c_size_t(0); ms = C.c_float(0); st = (C.c_uint64 * 8)()
        self._chk(self.lib.dg_bam_tags_finish(self.ctx, int(flags), C.byref(nb), st, C.byref(ms)), "dg_bam_tags_finish")
        self.bam_tags_stats, self.bam_tags_device_ms = tuple(int(x) for x in st), float(ms.value)
        split = (C.c_float * 2)()
        self._chk(self.lib.dg_bam_tags_device_ms(self.ctx, split), "dg_bam_tags_device_ms")
        self.bam_tags_device_ms_split = tuple(float(x) for x in split)
        return int(nb.value), self.bam_tags_stats

    def wait_index(self):
        self._chk(self.lib.dg_index_wait(self.ctx), "dg_index_wait")

    def init_report(self) -> str:
        return (self.lib.dg_init_report(self.ctx) or b"").decode()

    def clone(self):
        """A second context sharing this one's index on the same device (dg_clone): for a second batch in flight."""
        other = object.__new__(DartGPU)
        other.lib, other.index, other.params, other._parent = self.lib, self.index, self.params, self
        st = C.c_int(0)
        other.ctx = self.lib.dg_clone(self.ctx, C.byref(st))
        if not other.ctx:
            raise RuntimeError("dg_clone failed (%d): %s" % (st.value, (self.lib.dg_last_error(None) or b"").decode()))
        self._clones = getattr(self, "_clones", []) + [other]
        return other

    def close(self):
        for o in getattr(self, "_clones", []):
            o.close()
        self._clones = []
        if getattr(self, "ctx", None):
            self.lib.dg_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, (self.lib.dg_last_error(self.ctx) or b"").decode()))

    def set_params(self, params: Params):
        self.params = params
        self._chk(self.lib.dg_set_params(self.ctx, C.byref(params)), "dg_set_params")

    def upload(self, seq_off, rlen, flat):
        self._n = len(rlen)
        self._rlen_of_batch = np.asarray(rlen, np.uint16).copy()
        self._keep = (np.ascontiguousarray(seq_off, np.uint32), np.ascontiguousarray(rlen, np.uint16), np.ascontiguousarray(flat, np.uint8))
        a, b, c = self._keep
        self._chk(self.lib.dg_batch_upload(self.ctx, self._n, a.ctypes.data, b.ctypes.data, c.ctypes.data), "dg_batch_upload")

    def run(self):
        used = (C.c_size_t * 3)()
        self._chk(self.lib.dg_batch_run(self.ctx, used), "dg_batch_run")
        self._used = [int(x) for x in used]
        return self._used

    def download(self) -> BatchResult:
        u = self._used
        reads = np.zeros(self._n, dtype=READ_OUT)
        reports = np.zeros(max(u[0], 1), dtype=REPORT_OUT)
        cigar = np.zeros(max(u[1], 1), dtype=np.uint32)
        sj = np.zeros(max(u[2], 1), dtype=SJ_OUT)
        caps = (C.c_size_t * 3)(len(reports), len(cigar), len(sj))
        self._chk(self.lib.dg_batch_download(self.ctx, reads.ctypes.data, reports.ctypes.data, cigar.ctypes.data, sj.ctypes.data, caps), "dg_batch_download")
        return BatchResult(reads, reports[:u[0]], cigar[:u[1]], sj[:u[2]])

    def map_batch(self, seq_off, rlen, flat) -> BatchResult:
        self.upload(seq_off, rlen, flat)
        self.run()
        return self.download()

    def download_compact(self) -> BatchResult:
        """the records through the compact types (dg_batch_download_compact), expanded to the full dtypes"""
        u = self._used
        reads = np.zeros(self._n, dtype=READ_C); reports = np.zeros(max(u[0], 1), dtype=REPORT_C)
        cigar = np.zeros(max(u[1], 1), dtype=np.uint32); sj = np.zeros(max(u[2], 1), dtype=SJ_OUT)
        caps = (C.c_size_t * 3)(len(reports), len(cigar), len(sj))
        n_ops = C.c_size_t(0)
        self._chk(self.lib.dg_batch_download_compact(self.ctx, reads.ctypes.data, reports.ctypes.data, cigar.ctypes.data, sj.ctypes.data, caps, C.byref(n_ops)), "dg_batch_download_compact")
        self.last_compact_ops = int(n_ops.value)
        r, p, cg = expand_compact(reads, reports[:u[0]], cigar[:int(n_ops.value)], self._rlen_of_batch)
        return BatchResult(r, p, cg, sj[:u[2]])

    def upload_packed(self, words, nlist, rlen_all, rlen=None):
        self._n = int(words.shape[0])
        self._rlen_of_batch = np.full(self._n, rlen_all, np.uint16) if rlen is None else np.asarray(rlen, np.uint16).copy()
        w = np.ascontiguousarray(words, np.uint32); nl = np.ascontiguousarray(nlist, np.uint32)
        rl = None if rlen is None else np.ascontiguousarray(rlen, np.uint16)
        self._keep = (w, nl, rl)
        self._chk(self.lib.dg_batch_upload_packed(self.ctx, self._n, int(rlen_all), None if rl is None else rl.ctypes.data, int(w.shape[1]) if w.ndim == 2 else 1,
                                                  w.ctypes.data, nl.ctypes.data if len(nl) else None, len(nl)), "dg_batch_upload_packed")

    def map_batch_packed(self, words, nlist, rlen_all, rlen=None) -> BatchResult:
        self.upload_packed(words, nlist, rlen_all, rlen)
        self.run()
        return self.download()

    def map_batch_compact(self, words, nlist, rlen_all, rlen=None) -> BatchResult:
        """dg_map_batch_compact in one call: packed reads in, compact records out (built inside the run), expanded to the full dtypes;
        arrays sized by a guess and grown on DG_ERR_CAPACITY the way a C caller would"""
        n = int(words.shape[0])
        w = np.ascontiguousarray(words, np.uint32); nl = np.ascontiguousarray(nlist, np.uint32)
        rl = None if rlen is None else np.ascontiguousarray(rlen, np.uint16)
        self._n = n
        self._rlen_of_batch = np.full(n, rlen_all, np.uint16) if rl is None else rl.copy()
        cap = [n + n // 8 + 64, n // 4 + 64, 64]
        while True:
            reads = np.zeros(max(n, 1), dtype=READ_C); reports = np.zeros(cap[0], dtype=REPORT_C)
            cigar = np.zeros(cap[1], dtype=np.uint32); sj = np.zeros(cap[2], dtype=SJ_OUT)
            caps = (C.c_size_t * 3)(*cap); used = (C.c_size_t * 3)()
            rc = self.lib.dg_map_batch_compact(self.ctx, n, None, None if rl is None else rl.ctypes.data, None, int(rlen_all), int(w.shape[1]) if w.ndim == 2 else 1,
                                               w.ctypes.data, nl.ctypes.data if len(nl) else None, len(nl),
                                               reads.ctypes.data, reports.ctypes.data, cigar.ctypes.data, sj.ctypes.data, caps, used)
            u = [int(x) for x in used]
            if rc == -4:                                   # DG_ERR_CAPACITY: `used` holds the need (of what is known so far)
                cap = [max(cap[0], u[0] + 16), max(2 * cap[1], u[1] + 16), max(cap[2], u[2] + 16)]
                continue
            self._chk(rc, "dg_map_batch_compact")
            self._used = u
            r, p, cg = expand_compact(reads[:n], reports[:u[0]], cigar[:u[1]], self._rlen_of_batch)
            return BatchResult(r, p, cg, sj[:u[2]])

    def pinned(self, shape, dtype) -> "PinnedArray":
        return PinnedArray(self.lib, shape, dtype)

    def device_reads_tensor(self, compact: bool = False):
        """torch uint8 view [n_reads, 36] (or [n_reads, 16] of the compact type) of the per-read records in HBM (for RCCL collectives)."""
        import torch
        ptrs = (C.c_void_p * 4)()
        if compact:
            self._chk(self.lib.dg_batch_device_ptrs_compact(self.ctx, ptrs), "dg_batch_device_ptrs_compact")
        else:
            self._chk(self.lib.dg_batch_device_ptrs(self.ctx, ptrs), "dg_batch_device_ptrs")

        class _View:
            pass
        v = _View()
        v.__cuda_array_interface__ = {"shape": (self._n, READ_C.itemsize if compact else READ_OUT.itemsize), "typestr": "|u1", "data": (int(ptrs[0]), False), "version": 2}
        return torch.as_tensor(v, device="cuda")

    def device_records_compact(self):
        """the four compact record arrays of the last compact run as torch uint8 views of HBM (dg_batch_device_records_compact):
        [dg_read_c bytes, dg_report_c bytes, stored CIGAR ops bytes, dg_sj_out bytes] -- for the RCCL gather to the writing rank"""
        import torch
        ptrs = (C.c_void_p * 4)(); counts = (C.c_size_t * 4)()
        self._chk(self.lib.dg_batch_device_records_compact(self.ctx, ptrs, counts), "dg_batch_device_records_compact")
        out = []
        for k, item in enumerate((READ_C.itemsize, REPORT_C.itemsize, 4, SJ_OUT.itemsize)):
            nbytes = int(counts[k]) * item

            class _View:
                pass
            v = _View()
            if nbytes == 0 or not ptrs[k]:
                out.append(torch.empty(0, dtype=torch.uint8, device="cuda"))
                continue
            v.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptrs[k]), False), "version": 2}
            out.append(torch.as_tensor(v, device="cuda"))
        return out

    def timings(self):
        names = (C.c_char_p * 16)()
        ms = (C.c_float * 16)()
        n = self.lib.dg_last_timings(self.ctx, names, ms, 16)
        return [(names[i].decode(), float(ms[i])) for i in range(n)]

    def counters(self):
        out = (C.c_uint64 * 64)()
        n = self.lib.dg_last_counters(self.ctx, out, 64)
        keys = ["steps", "occ_blocks", "lf_steps", "sa_lookups", "seeds", "candidates", "nw_calls", "nw_cells", "reseed_calls", "reseed_window",
                "steps_executed", "occ_blocks_executed", "ktab_lookups", "lf_steps_executed", "direct_extensions", "k_seed_max_trips_per_read", "k_seed_wave_trips_max", "k_seed_wave_trips_sum", "k_reseed_trips", "k_reseed_wave_ticks_100mhz",
                "seedq_trips_begin", "seedq_trips_step", "seedq_trips_compare", "seedq_trips_locate", "seedq_trips_refill",
                "seedq_slots_begin", "seedq_slots_step", "seedq_slots_compare", "seedq_slots_locate", "seedq_slots_refill", "seedq_phases",
                "wave_ticks_k_seed_qf", "wave_ticks_k_seed_heavy", "wave_ticks_k_chain_heavy", "wave_ticks_k_pair", "wave_ticks_k_report", "general_path_units", "wave_chained_units", "batch_runs", "reruns_capacity_total", "reruns_scan_total",
                "k_reseed_windows_scanned_again_whole", "k_reseed_items", "k_reseed_chunks_through_pool"]
        return {keys[i]: int(out[i]) for i in range(min(n, len(keys)))}

    def probe_seeds(self, seq_off, rlen, flat):
        n = len(rlen)
        a, b, c = np.ascontiguousarray(seq_off, np.uint32), np.ascontiguousarray(rlen, np.uint16), np.ascontiguousarray(flat, np.uint8)
        cap = max(1024, n * 64)
        while True:
            so = np.zeros(n + 1, np.uint32); rp = np.zeros(cap, np.int32); sl = np.zeros(cap, np.int32); gp = np.zeros(cap, np.int64)
            used = C.c_size_t(0)
            rc = self.lib.dg_probe_seeds(self.ctx, n, a.ctypes.data, b.ctypes.data, c.ctypes.data, so.ctypes.data, rp.ctypes.data,
                                         sl.ctypes.data, gp.ctypes.data, cap, C.byref(used))
            if rc == -4:
                cap = int(used.value) + 16
                continue
            self._chk(rc, "dg_probe_seeds")
            u = int(used.value)
            return so, rp[:u], sl[:u], gp[:u]

    BGZF_PHASES = ("parse", "sort", "lengths", "codes", "header", "emit", "insert", "rest")

    def probe_bgzf_phases(self, data):
        """the dynamic BGZF kernel's clocks per phase on `data` (dg_probe_bgzf_phases) -> ({phase: cycles summed over strips and blocks}, BGZF bytes)"""
        a = np.ascontiguousarray(data, np.uint8) if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)
        cyc = (C.c_uint64 * 8)(); nb = C.c_size_t(0); ms = C.c_float(0)
        self._chk(self.lib.dg_probe_bgzf_phases(self.ctx, a.ctypes.data, len(a), cyc, C.byref(nb), C.byref(ms)), "dg_probe_bgzf_phases")
        self.bam_device_ms = float(ms.value)
        out = np.zeros(max(int(nb.value), 1), np.uint8)
        self._chk(self.lib.dg_batch_download_bam(self.ctx, out.ctypes.data, int(nb.value)), "dg_batch_download_bam")
        return dict(zip(self.BGZF_PHASES, (int(x) for x in cyc))), out[:int(nb.value)].tobytes()

    def probe_huff_lengths(self, freq, limit: int):
        """the code lengths the dynamic BGZF coder's builder gives a histogram, none above `limit`, computed on the device (dg_probe_huff_lengths)"""
        if not hasattr(self.lib, "dg_probe_huff_lengths"):
            raise RuntimeError("this build of libdartgpu.so has no dg_probe_huff_lengths")
        f = np.ascontiguousarray(freq, np.uint32)
        out = np.zeros(max(len(f), 1), np.uint8)
        self._chk(self.lib.dg_probe_huff_lengths(self.ctx, f.ctypes.data, len(f), int(limit), out.ctypes.data), "dg_probe_huff_lengths")
        return [int(x) for x in out[:len(f)]]

    def probe_refseq(self, g0: int, n: int) -> bytes:
        """RefSequence[g0, g0 + n) as the kernels read it from the device's text (dg_probe_refseq); 0 bytes outside [0, 2L)"""
        out = np.zeros(max(int(n), 1), np.uint8)
        self._chk(self.lib.dg_probe_refseq(self.ctx, int(g0), int(n), out.ctypes.data), "dg_probe_refseq")
        return out[:int(n)].tobytes()

    def probe_nw(self, pairs, mode: int = 0):
        """nw_alignment of (a, b) byte pairs through form `mode` of the kernels (dg_probe_nw_mode)."""
        n = len(pairs)
        a_off = np.zeros(n + 1, np.uint32); b_off = np.zeros(n + 1, np.uint32)
        for i, (x, y) in enumerate(pairs):
            a_off[i + 1] = a_off[i] + len(x); b_off[i + 1] = b_off[i] + len(y)
        a = np.frombuffer(b"".join(p[0] for p in pairs) + b"\0", dtype=np.uint8).copy()
        b = np.frombuffer(b"".join(p[1] for p in pairs) + b"\0", dtype=np.uint8).copy()
        cap = int(a_off[n]) + int(b_off[n]) + 16
        out_off = np.zeros(n + 1, np.uint32); out_len = np.zeros(n + 1, np.uint32)
        oa = np.zeros(cap, np.uint8); ob = np.zeros(cap, np.uint8)
        self._chk(self.lib.dg_probe_nw_mode(self.ctx, mode, n, a_off.ctypes.data, b_off.ctypes.data, a.ctypes.data, b.ctypes.data, out_off.ctypes.data,
                                            out_len.ctypes.data, oa.ctypes.data, ob.ctypes.data, cap), "dg_probe_nw_mode")
        res = []
        for i in range(n):
            o, l = int(out_off[i]), int(out_len[i])
            res.append((oa[o:o + l].tobytes(), ob[o:o + l].tobytes()))
        return res
