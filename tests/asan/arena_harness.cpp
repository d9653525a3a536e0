// TEST-ONLY: the bump cursor and the staging layout of orbslam2_amd/csrc/orbfe_arena.hpp under ASan + UBSan (tests/test_arena_asan.py).
// For each alignment / minimum pair the library uses -- 16 / 0 (staging blocks), 256 / 8 (lba_carve), 8 / 8 (eg_carve) -- fields of
// mixed types and counts (0, 1, odd) are carved twice, sizing and on an allocation of exactly bytes(), and every byte of every field
// is written: ASan is the judge of "inside".  lba_carve and eg_carve themselves need the HIP headers of their argument structs and are
// left to the GPU tests.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../orbslam2_amd/csrc/orbfe_arena.hpp"

static int checks = 0;
#define CHECK(c) do { checks++; if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

struct Rec28 { char b[28]; }; // a keypoint record: no power of two

struct Span { size_t off, bytes; };

// one field: carved, checked against the rules, filled
template <class T> static int carve(orbfe::Arena &sizing, orbfe::Arena &real, uint8_t *base, size_t align, size_t min_bytes, size_t count, std::vector<Span> &spans)
{
    const size_t before = sizing.bytes();
    CHECK(sizing.take<T>(count) == nullptr);
    T *p = real.take<T>(count);
    CHECK(p != nullptr);
    const size_t off = (size_t)((uint8_t *)p - base), want = sizeof(T) * count > min_bytes ? sizeof(T) * count : min_bytes;
    CHECK(off == before && off % align == 0);
    CHECK(sizing.bytes() == real.bytes() && sizing.bytes() == orbfe::round_up(off + want, align)); // a zero count takes its minimum
    memset(p, 0xA5, want);
    spans.push_back({off, want});
    return 0;
}

static int cursor(size_t align, size_t min_bytes, const std::vector<size_t> &counts)
{
    // pass 1 sizes with the same sequence of takes that pass 2 makes
    orbfe::Arena probe(nullptr, align, min_bytes);
    for (size_t n : counts) { probe.take<uint8_t>(n); probe.take<Rec28>(n); probe.take<double>(n); probe.take<int32_t>(3 * n + 1); }
    const size_t bytes = probe.bytes();
    CHECK(bytes > 0 && bytes % align == 0);
    void *mem = nullptr;
    CHECK(posix_memalign(&mem, align < sizeof(void *) ? sizeof(void *) : align, bytes) == 0);
    uint8_t *base = (uint8_t *)mem;
    orbfe::Arena sizing(nullptr, align, min_bytes), real(base, align, min_bytes);
    std::vector<Span> spans;
    int rc = 0;
    for (size_t n : counts) {
        rc = rc || carve<uint8_t>(sizing, real, base, align, min_bytes, n, spans) || carve<Rec28>(sizing, real, base, align, min_bytes, n, spans) ||
             carve<double>(sizing, real, base, align, min_bytes, n, spans) || carve<int32_t>(sizing, real, base, align, min_bytes, 3 * n + 1, spans);
    }
    if (!rc) {
        CHECK(sizing.bytes() == bytes && real.bytes() == bytes); // the same with and without a base
        for (size_t i = 0; i + 1 < spans.size(); i++) CHECK(spans[i].off + spans[i].bytes <= spans[i + 1].off); // in order, no overlap
        CHECK(spans.back().off + spans.back().bytes <= bytes);
    }
    free(mem);
    return rc;
}

static int cursor_overflow(size_t align, size_t min_bytes)
{
    uint8_t room[512];
    orbfe::Arena a(room, align, min_bytes);
    CHECK(a.take<int32_t>(4) != nullptr);
    const size_t before = a.bytes();
    CHECK(before != SIZE_MAX);
    CHECK(a.take<double>(SIZE_MAX / 4) == nullptr);  // the product does not fit
    CHECK(a.bytes() == SIZE_MAX);
    CHECK(a.take<uint8_t>(1) == nullptr);            // and stays refused
    orbfe::Arena b(nullptr, align, min_bytes);
    b.take<uint8_t>(64);
    b.take<uint8_t>(SIZE_MAX - 32);                  // the product fits, the sum does not
    CHECK(b.bytes() == SIZE_MAX);
    orbfe::Arena c(nullptr, align, min_bytes);
    c.take<uint8_t>(SIZE_MAX - 3);                   // the sum fits, its rounding does not
    CHECK(c.bytes() == SIZE_MAX);
    return 0;
}

template <class T> static int fill(uint8_t *base, size_t bytes, orbfe::Field<T> f, size_t count, size_t per)
{
    CHECK(f.offset % 16 == 0);
    CHECK(f.count == (count ? count : 1) * per);     // the padding belongs to the declaration
    CHECK(f.offset + sizeof(T) * f.count <= bytes);
    memset(base + f.offset, 0x5A, sizeof(T) * f.count);
    return 0;
}

static int layout(size_t n)
{
    orbfe::StageLayout L;
    CHECK(L.down() == 0 && L.bytes() == 0);
    const auto r0 = L.result<double>(8);
    const auto r1 = L.result<int32_t>(2);
    const auto r2 = L.result<float>(n, 16);
    const auto r3 = L.result<uint8_t>(n);
    const size_t down = L.down();
    CHECK(down == L.bytes());
    const auto i0 = L.input<Rec28>(n);
    const auto i1 = L.input<uint8_t>(n);
    const auto i2 = L.input<int32_t>(n + 1);
    const auto i3 = L.input<float>(n, 3);
    CHECK(L.down() == down && down <= i0.offset);    // the results end at or before the first input
    CHECK(r0.offset == 0 && r0.offset < r1.offset && r1.offset < r2.offset && r2.offset < r3.offset && r3.offset + r3.count <= down);
    CHECK(i0.offset < i1.offset && i1.offset < i2.offset && i2.offset < i3.offset);
    CHECK(r1.offset >= r0.offset + sizeof(double) * r0.count && r2.offset >= r1.offset + sizeof(int32_t) * r1.count && r3.offset >= r2.offset + sizeof(float) * r2.count);
    CHECK(i1.offset >= i0.offset + sizeof(Rec28) * i0.count && i2.offset >= i1.offset + i1.count && i3.offset >= i2.offset + sizeof(int32_t) * i2.count);
    const size_t bytes = L.bytes();
    CHECK(bytes % 16 == 0 && bytes != SIZE_MAX);
    uint8_t *base = (uint8_t *)malloc(bytes);
    CHECK(base != nullptr);
    const int rc = fill(base, bytes, r0, 8, 1) || fill(base, bytes, r1, 2, 1) || fill(base, bytes, r2, n, 16) || fill(base, bytes, r3, n, 1) ||
                   fill(base, bytes, i0, n, 1) || fill(base, bytes, i1, n, 1) || fill(base, bytes, i2, n + 1, 1) || fill(base, bytes, i3, n, 3);
    free(base);
    if (rc) return rc;
    bool refused = false;
    try { L.result<int32_t>(1); } catch (const std::logic_error &) { refused = true; }
    CHECK(refused);                                  // a result after an input
    CHECK(L.bytes() == bytes && L.down() == down);   // ... changes nothing
    return 0;
}

static int layout_overflow()
{
    orbfe::StageLayout L;
    L.result<int32_t>(4);
    L.input<double>(SIZE_MAX / 4);
    CHECK(L.bytes() == SIZE_MAX);
    orbfe::StageLayout M;
    M.result<uint8_t>(SIZE_MAX / 2, 3);              // count * per does not fit
    CHECK(M.bytes() == SIZE_MAX);
    return 0;
}

int main()
{
    const std::vector<size_t> counts = {0, 1, 7, 0, 33, 257, 1000, 0};
    const size_t rules[3][2] = {{16, 0}, {256, 8}, {sizeof(double), sizeof(double)}};
    for (const auto &r : rules)
        if (cursor(r[0], r[1], counts) || cursor_overflow(r[0], r[1])) return 1;
    for (size_t n : {(size_t)0, (size_t)1, (size_t)5, (size_t)1000})
        if (layout(n)) return 1;
    if (layout_overflow()) return 1;
    static_assert(orbfe::round_up(0, 16) == 0 && orbfe::round_up(1, 16) == 16 && orbfe::round_up(16, 16) == 16 && orbfe::round_up(17, 256) == 256, "round_up");
    printf("arena ok %d\n", checks);
    return 0;
}
