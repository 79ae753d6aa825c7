// pf_host.h -- internal, host code only: how many host threads a parallel section of the library may start; the build of
// the hash tables the text kernels probe.  Not part of the C ABI (include/panfeed_hip.h).
#pragma once

#include <cstdint>
#include <vector>

// std::thread::hardware_concurrency() says what the MACHINE has (256 on a GPU box whose container is given 16 CPUs by a
// CFS quota).  = min(hardware_concurrency, the affinity mask, TWICE the cgroup's cpu quota), at least 1; read once.
// Twice: measured on that box (round 5) the latency-bound sections are faster with 32 threads than with 16 -- more cache
// misses in flight -- and the rest indifferent; the quota still bounds a library dropped into a 2-CPU container.
// `cap`: the section's own upper bound.
unsigned pf_host_threads(unsigned cap);

// A table of 64-bit hashes, none of them 0: a power of two of slots, 0 = free, linear probing from hash & (slots - 1).
// Slots for n entries at a load of at most 1 / `load` (a slot stays free: every probe ends)
inline uint64_t pf_table_room(uint64_t n, uint64_t load) {
    uint64_t cap = 1024;
    while (cap < load * (n + 1)) cap <<= 1;
    return cap;
}

// h into the first free slot from its home on: -> that slot, for the caller to keep the entry's id by.  A slot on the way
// that holds an equal hash is shown to `same(slot)`; true: it IS this entry, nothing is put in, -> -1.  A set says true
// (equal hashes share a slot); a table whose entries are told apart by their bytes says false, or compares them itself
template <class Word, class Same> int64_t pf_table_insert(std::vector<Word>& hash, uint64_t h, Same&& same) {
    const uint64_t mask = hash.size() - 1;
    uint64_t slot = h & mask;
    for (; hash[slot] != 0; slot = (slot + 1) & mask)
        if (hash[slot] == h && same(slot)) return -1;
    hash[slot] = h;
    return (int64_t)slot;
}
