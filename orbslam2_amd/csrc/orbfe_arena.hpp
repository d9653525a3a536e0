// orbfe_arena.hpp -- how the host carves one buffer into typed fields: the bump cursor of the device scratch (lba_carve, eg_carve, the
// matchers' blocks) and the layout of the staging block of a synchronous entry point (StageBlock in orbfe_host.h copies it).  Plain
// C++17 without a HIP header: tests/asan/arena_harness.cpp runs it on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>

namespace orbfe {

// the one "round up to a power of two" of the host code
constexpr size_t round_up(size_t v, size_t pow2) { return (v + pow2 - 1) & ~(pow2 - 1); }

// Typed bump cursor over `base`; base == nullptr only sizes (every take returns null).  A field starts at a multiple of `align` (a
// power of two) and holds at least `min_bytes`.  Offsets are integers; a size that does not fit size_t makes bytes() SIZE_MAX, which
// no allocation grants, and every later take null.
class Arena {
public:
    Arena(void *base, size_t align, size_t min_bytes) : base_((uintptr_t)base), align_(align), min_(min_bytes) {}
    size_t take_bytes(size_t elem, size_t count) // the field's offset
    {
        size_t b, end;
        if (__builtin_mul_overflow(elem, count, &b)) overflow_ = true;
        if (b < min_) b = min_;
        if (__builtin_add_overflow(at_, b, &end) || end > SIZE_MAX - (align_ - 1)) overflow_ = true;
        const size_t o = at_;
        if (!overflow_) at_ = round_up(end, align_);
        return o;
    }
    template <class T> T *take(size_t count)
    {
        const size_t o = take_bytes(sizeof(T), count);
        return base_ && !overflow_ ? reinterpret_cast<T *>(base_ + o) : nullptr;
    }
    size_t bytes() const { return overflow_ ? SIZE_MAX : at_; }

private:
    uintptr_t base_;
    size_t align_, min_, at_ = 0;
    bool overflow_ = false;
};

// a field of a staging block: `count` elements of T at byte `offset`
template <class T> struct Field {
    size_t offset = 0, count = 0;
};

// The block of a synchronous entry point: results first -- [0, down()) is what comes back in one copy -- then the inputs.  What is
// uploaded and read back (a pose, an outlier flag) is a result.  A field holds per * max(count, 1) elements, so an empty array still
// has an address of its own, and starts at a multiple of 16.
class StageLayout {
public:
    template <class T> Field<T> result(size_t count, size_t per = 1)
    {
        if (inputs_) throw std::logic_error("staging layout: a result declared after an input");
        const Field<T> f = field<T>(count, per);
        down_ = cur_.bytes();
        return f;
    }
    template <class T> Field<T> input(size_t count, size_t per = 1)
    {
        inputs_ = true;
        return field<T>(count, per);
    }
    size_t down() const { return down_; }
    size_t bytes() const { return cur_.bytes(); }

private:
    template <class T> Field<T> field(size_t count, size_t per)
    {
        size_t n;
        if (__builtin_mul_overflow(count ? count : 1, per, &n)) n = SIZE_MAX; // the cursor then overflows as well
        return {cur_.take_bytes(sizeof(T), n), n};
    }
    Arena cur_{nullptr, 16, 0};
    size_t down_ = 0;
    bool inputs_ = false;
};

} // namespace orbfe
