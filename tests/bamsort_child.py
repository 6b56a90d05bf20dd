"""Child process of tests/test_gpu_bam_sort.py: started with DG_BAMSORT_FIRST_CAP in its environment, so every context's store begins tiny and grows while
the batches arrive.  usage: bamsort_child.py <index prefix> <reads.npz> <output>; prints one JSON line with the growth counts."""
import json, os, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from dart_amd import host  # noqa: E402


def main(prefix, npz, out):
    z = np.load(npz)
    reads, headers, quals, p = z["reads"], [str(x) for x in z["headers"]], [str(x) for x in z["quals"]], json.loads(str(z["p"]))
    gpu = host.DartGPU(host.Index(prefix))
    clone = gpu.clone()
    n = len(reads)
    cuts = [0, 600, 1200, 1800, 2400, n]
    # ordinals in read order, calls shuffled, two contexts; each store starts at its first batch's size and doubles: the clone's grows at its second and at
    # its third batch, the parent's at its second batch and at the merge
    for k, g in ((1, clone), (4, gpu), (0, clone), (2, gpu), (3, clone)):
        lo, hi = cuts[k], cuts[k + 1]
        so, rl, flat = host.pack_reads(reads[lo:hi])
        g.set_params(host.default_params(paired=1, **p))
        g.map_batch(so, rl, flat)
        g.format_bam(headers[lo:hi], quals[lo:hi], hi - lo, raw=True)
        g.accumulate_bam(k)
    clone_growths = clone.bam_sort_info()["growths"]
    gpu.bam_sort_merge(clone)
    n_rec, nb = gpu.bam_sort_finish()
    open(out, "wb").write(gpu.bam_sort_compress(0, nb, raw=True))
    print(json.dumps(dict(records=n_rec, bytes=nb, growths=gpu.bam_sort_info()["growths"], clone_growths=clone_growths)))
    gpu.close()


if __name__ == "__main__":
    main(*sys.argv[1:4])
