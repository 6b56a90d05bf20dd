"""What the tests of tests/read_structures.py's classes share: the two committed read sets (over the golden genomes, so no new index),
the flag sets they run under, and small helpers over the oracle's records."""
from __future__ import annotations

import gzip, json, os
import numpy as np
import common, read_structures as rs
from dart_amd import host

SEED = 20261
N_PER_CLASS = 70                                   # (the committed SAM and stage dump of the 101-base set stay within the size of the largest fixture)
SETS = {"rs101": ("pe101_spliced", 101), "rs250": ("pe151_spliced", 250)}
FLAG_SETS = (["-mis", "5"], ["-mis", "12", "-m"], ["-mis", "30"])
# The 250-base set holds the classes that only fit such reads (three_junctions, ins_31_80).  Inserted bases count against -mis, so an insertion of 31-80 bases maps under no
# flag set above: the 250-base set also runs at -mis 100, under which the wave-wide alignment's result for segment pairs wider than 64 columns reaches the records.
WIDE_FLAGS = ["-mis", "100"]
SET_FLAGS = {"rs101": FLAG_SETS, "rs250": FLAG_SETS + (WIDE_FLAGS,)}              # what the lane programs on the host run
REF_FLAGS = {"rs101": FLAG_SETS, "rs250": (["-mis", "30"], WIDE_FLAGS)}           # the runs of the reference's object code that tests/golden/read_structures.json records
ALL_SJ_FLAGS = ["-mis", "5", "-all_sj", "-max_dup", "1000"]
GPU_FLAG_SETS = {name: flags + (ALL_SJ_FLAGS,) for name, flags in SET_FLAGS.items()}
FIXTURE_FLAGS = ["-mis", "12", "-m"]               # the run whose SAM, junctions and stage dump are committed (tests/golden/read_structures.mis12m.*)
GOLD = os.path.join(common.GOLDEN, "read_structures.json")
BASE = os.path.join(common.GOLDEN, "read_structures.mis12m")
# With -m a pair's lines show every report of positive score, but for a read that maps uniquely SetPairedAlignmentFlag (Mapping.cpp:106-121) sets the flag of its best
# report alone: the reference prints the other reports' iFrag as the heap left it (one read of the 101-base set: a chimera whose halves both align; the printed FLAG
# changes from run to run).  The oracle and the library zero the field.  The reference's object code therefore runs with glibc's MALLOC_PERTURB_=255 here, which
# hands out zeroed blocks, so that the field it never wrote reads as 0 in every run.
REF_ENV = dict(os.environ, MALLOC_PERTURB_="255")
_sets = {}
OPS = "MIDNSHP=X"


def read_set(name, workdir):
    """-> (golden case, {class: pairs}, {class: info})"""
    if name not in _sets:
        case, rlen = SETS[name]
        c = common.build_case(case, workdir)
        classes, info = rs.make_with_info(c["genome"], SEED, rlen, N_PER_CLASS)
        _sets[name] = (c, classes, info)
    return _sets[name]


def gold():
    return json.load(open(GOLD))


def run_key(name, flags):
    return name + ": " + " ".join(flags)


def fixture_sam():
    return gzip.open(BASE + ".sam.gz", "rt").read()


def fixture_junctions():
    return open(BASE + ".junctions.tab").read()


def cigar_lists(rep, cig):
    """per report: [(length, operation character)]"""
    out = []
    for r in rep:
        ops = cig[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])]
        out.append([(int(x) >> 4, OPS[int(x) & 15]) for x in ops])
    return out


def best_cigars(reads, rep, cig):
    """per read: the CIGAR of its best report as [(length, op)], or None where the read is unmapped"""
    cl = cigar_lists(rep, cig)
    out = []
    for r in reads:
        k = int(r["rep_off"]) + max(int(r["best"]), 0)
        out.append(None if int(r["score"]) == 0 else cl[k])
    return out


def padded_2bit(reads):
    """reads of several lengths (A/C/G/T/N only) -> (words, nlist, longest length, lengths) for the packed entry points"""
    n = max(len(r) for r in reads)
    arr = np.full((len(reads), n), ord("A"), np.uint8)
    for i, r in enumerate(reads):
        arr[i, :len(r)] = np.frombuffer(r, np.uint8)
    words, nlist = host.pack_reads_2bit(arr)
    return words, nlist, n, np.asarray([len(r) for r in reads], np.uint16)
