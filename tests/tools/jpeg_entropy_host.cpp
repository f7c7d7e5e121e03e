// jpeg_entropy_host.cpp -- csrc/jpeg_entropy.h on the host: the decoder's marker walk, table builder, bit reader and block decoder run
// over the files of a directory, from buffers of exactly the files' size into buffers of exactly the needed size, so that the host
// sanitizers see every access (tests/test_jpeg_decode_cpu.py builds this with -fsanitize=address,undefined).  The restart scan and
// the merge of the intervals' statuses are restated here as plainly as possible; on the device they are jpeg_decode.hip's kernels.
//
//   jpeg_entropy_host DIR LIST   ->   one line per line "name H W C" of LIST:   name status intervals checksum-of-the-coefficients
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "jpeg_entropy.h"

using namespace soar::jpgd;

namespace {

struct Result {
    int32_t status = 0, intervals = 0;
    uint32_t checksum = 0;
};

Result decode_file(const uint8_t *f, int64_t L, int H, int W, int C)
{
    Result res;
    Rec *r = new Rec;
    std::vector<int64_t> marks;
    int16_t *coef = nullptr;
    res.status = parse(f, L, H, W, C, *r);
    if (res.status == JPEG_OK) {
        r->has_end = 0;
        r->seg_end = L;
        bool sequence = true;
        for (int64_t p = r->scan; p + 1 < L; p++) {
            if (!marker_at(f, L, p)) continue;
            if (f[p + 1] < 0xD0 || f[p + 1] > 0xD7) { r->has_end = 1; r->seg_end = p; break; }
            if (f[p + 1] != 0xD0 + (int)(marks.size() & 7)) sequence = false;
            marks.push_back(p);
        }
        res.status = intervals_of(*r, (int64_t)marks.size());
        if (res.status == JPEG_OK && !sequence) res.status = JPEG_CORRUPT;
    }
    if (res.status == JPEG_OK) {
        res.intervals = r->n_int;
        const size_t count = (size_t)r->blocks * 64;
        coef = (int16_t *)calloc(count, sizeof(int16_t));       // exactly sized: an access beyond it is the sanitizer's to report
        const int32_t per = r->ri ? r->ri : r->mcus;
        for (int32_t j = 0; j < r->n_int; j++) {
            const int64_t start = j ? marks[j - 1] + 2 : r->scan, end = j < r->n_int - 1 ? marks[j] : r->seg_end;
            const int32_t mcu0 = j * per, n = r->mcus - mcu0 < per ? r->mcus - mcu0 : per;
            const int32_t st = decode_interval(f, *r, coef, start, end, mcu0, n, j == r->n_int - 1 && !r->has_end);
            if (st != JPEG_OK && (res.status == JPEG_OK || st < res.status)) res.status = st;
        }
        if (res.status == JPEG_OK)
            for (size_t i = 0; i < count; i++) res.checksum += ((uint32_t)(uint16_t)coef[i] * (uint32_t)((i * 31 + 7) & 0xFFFF));
        free(coef);
    }
    delete r;
    return res;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s DIR LIST\n", argv[0]); return 2; }
    FILE *list = fopen(argv[2], "r");
    if (!list) { perror(argv[2]); return 2; }
    char name[256];
    int H, W, C;
    while (fscanf(list, "%255s %d %d %d", name, &H, &W, &C) == 4) {
        const std::string path = std::string(argv[1]) + "/" + name;
        FILE *fp = fopen(path.c_str(), "rb");
        if (!fp) { perror(path.c_str()); return 2; }
        std::vector<uint8_t> bytes;
        uint8_t buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, fp)) > 0) bytes.insert(bytes.end(), buf, buf + got);
        fclose(fp);
        uint8_t *f = (uint8_t *)malloc(bytes.size() ? bytes.size() : 1);     // exactly sized
        if (!bytes.empty()) memcpy(f, bytes.data(), bytes.size());
        const Result r = decode_file(bytes.empty() ? f + 1 : f, (int64_t)bytes.size(), H, W, C);
        printf("%s %d %d %08x\n", name, r.status, r.intervals, r.checksum);
        free(f);
    }
    fclose(list);
    return 0;
}
