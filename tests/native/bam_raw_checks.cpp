// CPU suite: the expected bytes of the device's BAM records -- BamWriter::sam_line_to_bam (dart_amd/csrc/host/bam_writer.h) over every line of a SAM
// body, the results concatenated.  argv[1]: the chromosome names, one per line; argv[2]: the SAM body; argv[3]: out.  Prints "records=N refused=M".
#include "bam_writer.h"
#include <fstream>
#include <sstream>

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    std::vector<std::string> names; std::vector<int64_t> lens;
    { std::ifstream f(argv[1]); std::string l; while (std::getline(f, l)) { names.push_back(l); lens.push_back(1000); } }
    std::string text;
    { std::ifstream f(argv[2], std::ios::binary); std::stringstream ss; ss << f.rdbuf(); text = ss.str(); }
    BamWriter w;
    const std::string scratch = std::string(argv[3]) + ".header";       // (open() is what fills the writer's table of names)
    if (!w.open(scratch.c_str(), "", names, lens, 1)) return 2;
    std::vector<uint8_t> all, one;
    long long good = 0, refused = 0;
    const char *p = text.data(), *end = p + text.size();
    while (p < end) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
        const char *le = nl ? nl : end;
        if (le > p) {
            one.clear();
            if (w.sam_line_to_bam(p, (size_t)(le - p), one)) { all.insert(all.end(), one.begin(), one.end()); good++; } else refused++;
        }
        p = nl ? nl + 1 : end;
    }
    w.close();
    FILE *o = fopen(argv[3], "wb");
    if (!o) return 2;
    if (!all.empty() && fwrite(all.data(), 1, all.size(), o) != all.size()) return 2;
    fclose(o);
    printf("records=%lld refused=%lld\n", good, refused);
    return 0;
}
