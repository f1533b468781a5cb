// CPU check of crcnn_amd/csrc/work_arena.h: for random lists of regions, the counting run and the carving run of the same list agree, on a host buffer of exactly
// bytes() at every offset 0 .. 255 from a 256-byte boundary.  Built with -fsanitize=address,undefined (tests/test_work_arena_cpu.py): every byte of every
// region is written, so a region past the buffer's end is an error the sanitizer reports.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <utility>
#include <vector>
#include "work_arena.h"

struct Region { int kind; size_t count; };      // kind: the element type the region is taken as

// the same list of take<T>() calls on either arena; returns {start, byte length} of every region
static std::vector<std::pair<uintptr_t, size_t>> run(WorkArena &a, const std::vector<Region> &regions)
{
    std::vector<std::pair<uintptr_t, size_t>> out;
    for (const Region &r : regions) {
        switch (r.kind) {
        case 0: out.push_back({(uintptr_t)a.take<signed char>(r.count), r.count}); break;
        case 1: out.push_back({(uintptr_t)a.take<int>(r.count), r.count * sizeof(int)}); break;
        default: out.push_back({(uintptr_t)a.take<uint64_t>(r.count), r.count * sizeof(uint64_t)}); break;
        }
    }
    return out;
}

#define REQUIRE(x) do { if (!(x)) { std::printf("FAILED %s (line %d, list %d, offset %d)\n", #x, __LINE__, list, off); return 1; } } while (0)

int main()
{
    std::mt19937_64 rng(20240229);
    long checked = 0;
    for (int list = 0; list < 400; list++) {
        int off = -1;
        std::vector<Region> regions(list == 0 ? 0 : 1 + rng() % 7);
        // sizes around the alignment: empty regions, one element, just under / at / just over a multiple of 256 bytes, and larger odd ones
        for (Region &r : regions) {
            r.kind = (int)(rng() % 3);
            const size_t picks[] = {0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, (size_t)(rng() % 5000)};
            r.count = picks[rng() % (sizeof(picks) / sizeof(picks[0]))];
        }
        WorkArena counting;
        for (const auto &pr : run(counting, regions)) REQUIRE(pr.first == 0);         // a counting arena hands out no pointers
        const size_t bytes = counting.bytes();
        REQUIRE(bytes >= 256);
        for (off = 0; off < 256; off++) {
            // a buffer that starts `off` bytes past a 256-byte boundary and ends exactly bytes() later: the sanitizer guards what follows
            void *raw = nullptr;
            REQUIRE(posix_memalign(&raw, 256, off + bytes) == 0);
            unsigned char *d_work = (unsigned char *)raw + off;
            WorkArena carving(d_work);
            const auto got = run(carving, regions);
            REQUIRE(carving.bytes() <= bytes);                                          // counting >= carving extent
            for (size_t i = 0; i < got.size(); i++) {
                REQUIRE(got[i].first % 256 == 0);
                REQUIRE(got[i].first >= (uintptr_t)d_work && got[i].first + got[i].second <= (uintptr_t)d_work + bytes);
                for (size_t j = 0; j < i; j++)
                    REQUIRE(got[j].first + got[j].second <= got[i].first || got[i].first + got[i].second <= got[j].first || !got[i].second || !got[j].second);
                std::memset((void *)got[i].first, (int)(i + 1), got[i].second);         // the sanitizer sees an overrun of the allocation
            }
            // every region still holds its own fill: nothing was written twice
            for (size_t i = 0; i < got.size(); i++)
                for (size_t b = 0; b < got[i].second; b++) REQUIRE(((unsigned char *)got[i].first)[b] == (unsigned char)(i + 1));
            std::free(raw);
            checked++;
        }
    }
    std::printf("ok %ld\n", checked);
    return 0;
}
