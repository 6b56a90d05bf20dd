// tests/native/bam_writer_offset_checks.cpp -- BamWriter::first_block_offset (dart_amd/csrc/host/bam_writer.h) is counted from the blocks the writer hands to
// the file, never sought: `-bo` on a pipe must work as it always did.  usage: bam_writer_offset_checks <output>; prints "ok <0|1> first <offset>" to stderr
#include "bam_writer.h"

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: bam_writer_offset_checks <output>\n"); return 1; }
    BamWriter w;
    std::string text = "@PG\tID:dart\n";
    for (int k = 0; k < 8000; k++) text += "@CO\tline " + std::to_string(k * 2654435761u) + "\n";        // a header of more than one block
    const bool ok = w.open(argv[1], text, {"chr1", "chr2"}, {300000, 200000}, 2);
    const unsigned long long first = (unsigned long long)w.first_block_offset();
    const std::string line = "r1\t0\tchr1\t100\t60\t5M\t*\t0\t0\tACGTA\tIIIII\tNM:i:0\n";
    w.add_sam_text(line.data(), line.size());
    const bool closed = ok && w.close();
    fprintf(stderr, "ok %d first %llu\n", (int)(ok && closed), first);
    return ok && closed ? 0 : 2;
}
