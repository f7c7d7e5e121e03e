// png_inflate_host.cpp -- csrc/png_inflate.h on the host: the decoder's bit reader, table builder and symbol decoder run over every file
// of a directory, into buffers of exactly the needed size, so that the host sanitizers see every access (tests/test_png_decode_cpu.py
// builds this with -fsanitize=address,undefined).  The chunk walk, the segment rule and the checks around the decoder are restated
// here as plainly as possible; on the device they are png_decode.hip's kernels.
//
//   png_inflate_host DIR   ->   one line per file, in name order:   name status segments adler32-of-the-filtered-stream
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dirent.h>
#include <string>
#include <vector>

#include "png_inflate.h"

using namespace soar::pngi;

namespace {

// the host's sink: bytes into out[0, cap)
struct ByteSink {
    uint8_t *out;
    int64_t cap, pos;
    bool lit(uint8_t v)
    {
        if (pos >= cap) return false;
        out[pos++] = v;
        return true;
    }
    int32_t match(uint32_t dist, uint32_t len)
    {
        if ((int64_t)dist > pos) return PNG_CORRUPT;
        if (pos + (int64_t)len > cap) return PNG_WRONG_LENGTH;
        for (uint32_t i = 0; i < len; i++, pos++) out[pos] = out[pos - dist];
        return PNG_OK;
    }
    int32_t stored(const uint8_t *z, int64_t from, uint32_t len)
    {
        if (pos + (int64_t)len > cap) return PNG_WRONG_LENGTH;
        if (len) memcpy(out + pos, z + from, len);
        pos += len;
        return PNG_OK;
    }
    void finish() {}
};

uint32_t crc32(const uint8_t *p, size_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    }
    return ~c;
}

uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

struct Result {
    int32_t status = 0, segments = 1;
    uint32_t adler = 0;
};

Result decode_file(const std::vector<uint8_t> &f)
{
    Result r;
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    const int64_t L = (int64_t)f.size();
    if (L < 8 || memcmp(f.data(), sig, 8)) { r.status = PNG_BAD_STRUCTURE; return r; }
    std::vector<uint8_t> z;
    std::vector<int64_t> starts;                                 // the segments' first bytes in z
    int64_t H = 0, W = 0, C = 0, pos = 8;
    bool first = true, idat = false, prev_stored = false;
    for (;;) {
        if (pos + 12 > L) { r.status = PNG_BAD_STRUCTURE; return r; }
        const uint8_t *c = f.data() + pos;
        const int64_t len = be32(c);
        if (len > 0x7FFFFFFF || pos + 12 + len > L) { r.status = PNG_BAD_STRUCTURE; return r; }
        const bool crc_ok = crc32(c + 4, (size_t)len + 4) == be32(c + 8 + len);
        if (first) {
            if (memcmp(c + 4, "IHDR", 4) || len != 13) { r.status = PNG_BAD_STRUCTURE; return r; }
            if (!crc_ok) { r.status = PNG_BAD_CRC; return r; }
            W = be32(c + 8);
            H = be32(c + 12);
            if (W == 0 || H == 0 || W > 0x7FFFFFFF || H > 0x7FFFFFFF) { r.status = PNG_BAD_STRUCTURE; return r; }
            const int colour = c[17];
            if (c[16] != 8 || (colour != 0 && colour != 2 && colour != 6) || c[18] || c[19] || c[20]) { r.status = PNG_UNSUPPORTED; return r; }
            C = colour == 0 ? 1 : (colour == 2 ? 3 : 4);
            first = false;
        } else if (!memcmp(c + 4, "IHDR", 4)) {
            r.status = PNG_BAD_STRUCTURE;
            return r;
        } else if (!memcmp(c + 4, "IDAT", 4)) {
            if (!crc_ok) { r.status = PNG_BAD_CRC; return r; }
            // a candidate: behind 00 00 FF FF, or behind an IDAT that is exactly one stored block
            const int64_t p = (int64_t)z.size();
            if (idat && p >= 6 && ((z[p - 4] == 0 && z[p - 3] == 0 && z[p - 2] == 0xFF && z[p - 1] == 0xFF) || prev_stored) &&
                (starts.empty() || starts.back() < p))
                starts.push_back(p);
            z.insert(z.end(), c + 8, c + 8 + len);
            const int64_t a = p == 0 ? 2 : p, b = (int64_t)z.size();
            prev_stored = b - a >= 5 && z[a] == 0 && (z[a + 1] ^ z[a + 3]) == 0xFF && (z[a + 2] ^ z[a + 4]) == 0xFF &&
                          b - a == 5 + z[a + 1] + 256 * z[a + 2];
            idat = true;
        } else if (!memcmp(c + 4, "IEND", 4)) {
            break;
        } else if (!(c[4] & 0x20) && memcmp(c + 4, "PLTE", 4)) {
            r.status = PNG_UNSUPPORTED;                          // a critical chunk this decoder does not know
            return r;
        }
        pos += 12 + len;
    }
    if (!idat) { r.status = PNG_BAD_STRUCTURE; return r; }
    const int64_t S = H * (1 + W * C), n = (int64_t)z.size();
    if (S > 0x7FFFFFFF) { r.status = PNG_UNSUPPORTED; return r; }
    if (n < 2) { r.status = PNG_CORRUPT; return r; }
    if ((r.status = zlib_header(z[0], z[1])) != 0) return r;
    while (!starts.empty() && starts.back() >= n) starts.pop_back();     // (a candidate needs a byte of its own)
    starts.insert(starts.begin(), 2);

    // exactly sized copies: an access beyond either is the sanitizer's to report
    uint8_t *zz = (uint8_t *)malloc((size_t)n), *out = (uint8_t *)malloc((size_t)S);
    memcpy(zz, z.data(), (size_t)n);
    Tables *t = new Tables;
    const size_t ns = starts.size();
    std::vector<int64_t> lens(ns, -1);
    bool parallel = ns > 1;
    int64_t sum = 0;
    for (size_t k = 0; parallel && k < ns; k++) {                // the first pass: every candidate from its byte, nothing written
        const bool last = k + 1 == ns;
        Bits br(zz, last ? n : starts[k + 1], starts[k]);
        CountSink cs(S);
        if (inflate(br, *t, cs, last) != 0) parallel = false;
        lens[k] = cs.pos;
        sum += cs.pos;
    }
    if (parallel && sum != S) parallel = false;
    if (parallel) {
        r.segments = 0;                                          // the segments that give bytes (the encoder's last IDAT gives none)
        for (size_t k = 0; k < ns; k++) r.segments += lens[k] > 0;
        int64_t at = 0;
        for (size_t k = 0; k < ns && r.status == 0; k++) {
            const bool last = k + 1 == ns;
            Bits br(zz, last ? n : starts[k + 1], starts[k]);
            ByteSink bs{out + at, lens[k], 0};
            r.status = inflate(br, *t, bs, last);
            if (r.status == 0 && bs.pos != lens[k]) r.status = PNG_WRONG_LENGTH;
            at += lens[k];
        }
    } else {
        Bits br(zz, n, 2);
        ByteSink bs{out, S, 0};
        r.status = inflate(br, *t, bs, true);
        if (r.status == 0 && bs.pos != S) r.status = PNG_WRONG_LENGTH;
    }
    if (r.status == 0) {
        uint32_t a = 1, b = 0;
        for (int64_t i = 0; i < S; i++) { a = (a + out[i]) % 65521u; b = (b + a) % 65521u; }
        r.adler = b << 16 | a;
        if (r.adler != be32(zz + n - 4)) r.status = PNG_BAD_ADLER;
    }
    for (int64_t y = 0; r.status == 0 && y < H; y++)
        if (out[y * (1 + W * C)] > 4) r.status = PNG_BAD_FILTER;
    if (r.status) r.adler = 0;
    delete t;
    free(zz);
    free(out);
    return r;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
    std::vector<std::string> names;
    DIR *d = opendir(argv[1]);
    if (!d) { perror(argv[1]); return 2; }
    while (dirent *e = readdir(d))
        if (e->d_name[0] != '.') names.push_back(e->d_name);
    closedir(d);
    std::sort(names.begin(), names.end());
    for (const std::string &name : names) {
        const std::string path = std::string(argv[1]) + "/" + name;
        FILE *fp = fopen(path.c_str(), "rb");
        if (!fp) { perror(path.c_str()); return 2; }
        std::vector<uint8_t> f;
        uint8_t buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, fp)) > 0) f.insert(f.end(), buf, buf + got);
        fclose(fp);
        const Result r = decode_file(f);
        printf("%s %d %d %08x\n", name.c_str(), r.status, r.segments, r.adler);
    }
    return 0;
}
