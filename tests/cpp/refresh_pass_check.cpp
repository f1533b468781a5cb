// refresh_pass_check.cpp -- refresh_pass_len (crcnn_amd/host/refresh_pass.h) against the two pass-length computations it replaced, written out here as the four
// refresh drivers had them, and a model of the driver's loop: every item visited once, the keystream ids of the passes contiguous.  No engine, no device.
#include "refresh_pass.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s (line %d): one %zu items %zu in_cts %zu\n", #x, __LINE__, one, items, in_cts); return 1; } } while (0)

// refreshImages, rescaleSlots, rescaleSlotsCrt: a pass of ciphertexts
static size_t pass_of_ciphertexts(size_t one, size_t cnt)
{
    size_t pass = ((size_t)4 << 30) / (one ? one : 1);
    if (pass < 1024) pass = 1024;
    if (pass > cnt) pass = cnt;
    return pass;
}
// actSlots: a pass of whole planes of in_cts ciphertexts
static size_t pass_of_planes(size_t one, size_t planes, size_t in_cts)
{
    size_t pass = ((size_t)4 << 30) / (one ? one : 1);
    if (pass * in_cts < 1024) pass = (1024 + in_cts - 1) / in_cts;
    if (pass > planes) pass = planes;
    return pass;
}

int main()
{
    const size_t MiB4 = (size_t)4 << 20;
    const size_t ones[] = {0, 1, MiB4 - 8, MiB4, MiB4 + 8, ((size_t)4 << 30) + 1}, counts[] = {0, 1, 1023, 1024, 1025, 10000000}, per_item[] = {1, 25, 1024};
    size_t cases = 0, passes = 0;
    for (size_t one : ones) for (size_t items : counts) for (size_t in_cts : per_item) {
        const size_t pass = refresh_pass_len(one, items, in_cts);
        CHECK(pass == pass_of_planes(one, items, in_cts));
        if (in_cts == 1) CHECK(pass == pass_of_ciphertexts(one, items));
        CHECK(pass <= items && (pass >= 1 || items == 0));
        // the driver's loop, with ids keystream ids per item (the outputs of an item; r per ciphertext for a CRT base) from a counter that starts anywhere
        for (size_t ids : {(size_t)1, (size_t)4, (size_t)9}) {
            const uint64_t start = 0xfffffffffff00000ull * (ids - 1) + 77;
            uint64_t counter = start;
            size_t next_item = 0;
            for (size_t o = 0; o < items; o += pass, passes++) {
                const size_t c = pass < items - o ? pass : items - o;
                CHECK(o == next_item && c >= 1);                               // no item skipped, none visited twice
                CHECK(counter == start + (uint64_t)o * ids);                   // this pass draws [counter, counter + c ids): no gap, no overlap
                next_item = o + c; counter += (uint64_t)c * ids;
            }
            CHECK(next_item == items && counter == start + (uint64_t)items * ids);
        }
        cases++;
    }
    std::printf("ok %zu cases %zu passes\n", cases, passes);
    return 0;
}
