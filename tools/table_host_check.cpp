// table_host_check.cpp -- a stand-alone check of the host's hash-table build (csrc/pf_host.h: pf_table_room,
// pf_table_insert), for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/table_host_check.cpp \
//       -o /tmp/table_host_check && /tmp/table_host_check
// The three users' ways of inserting -- a set (equal hashes share a slot), entries with ids (equal hashes take slots of
// their own), and ids with duplicates left out by a compare -- over no key, one key, duplicate keys, two keys forced to
// the same slot, a run that wraps round the end of the table, and a table filled to its load.  Exit status 0: all as expected.
#include "../panfeed_amd/csrc/pf_host.h"

#include <cstdio>
#include <string>

namespace {
int failures = 0, checks = 0;
void expect(bool ok, const char* what) { checks++; if (!ok) { failures++; fprintf(stderr, "FAIL %s\n", what); } }

const auto SHARE = [](uint64_t) { return true; };
const auto OWN = [](uint64_t) { return false; };
uint64_t used(const std::vector<uint64_t>& t) { uint64_t n = 0; for (uint64_t h : t) n += h != 0; return n; }
}  // namespace

int main() {
    // room: 1 024 slots at least, a power of two, load * (n + 1) slots at least
    expect(pf_table_room(0, 4) == 1024 && pf_table_room(0, 2) == 1024, "room for nothing");
    expect(pf_table_room(255, 4) == 1024 && pf_table_room(256, 4) == 2048, "room at load 4");
    expect(pf_table_room(511, 2) == 1024 && pf_table_room(512, 2) == 2048, "room at load 2");
    expect(pf_table_room((1ull << 24) - 1, 2) == 1ull << 25, "room for 2^24 - 1 strains");

    {   // empty input: a table of free slots
        std::vector<uint64_t> t(pf_table_room(0, 4), 0);
        expect(used(t) == 0 && t.size() == 1024, "empty table");
    }
    {   // one key: its home slot; the same key again: shared (a set), or a slot of its own behind it
        std::vector<uint64_t> t(1024, 0);
        expect(pf_table_insert(t, 5 + 3 * 1024, SHARE) == 5 && t[5] == 5 + 3 * 1024 && used(t) == 1, "one key");
        expect(pf_table_insert(t, 5 + 3 * 1024, SHARE) == -1 && used(t) == 1, "duplicate key in a set");
        expect(pf_table_insert(t, 5 + 3 * 1024, OWN) == 6 && t[6] == t[5] && used(t) == 2, "equal hashes, own slots");
    }
    {   // two different hashes forced to the same slot: the second goes behind the first, in either mode
        for (int own = 0; own < 2; own++) {
            std::vector<uint64_t> t(1024, 0);
            auto ins = [&](uint64_t h) { return own ? pf_table_insert(t, h, OWN) : pf_table_insert(t, h, SHARE); };
            expect(ins(7) == 7 && ins(7 + 1024) == 8 && ins(8) == 9 && t[7] == 7 && t[8] == 7 + 1024 && t[9] == 8, "same home slot");
        }
    }
    {   // the run wraps round the end of the table
        std::vector<uint64_t> t(1024, 0);
        expect(pf_table_insert(t, 1023, OWN) == 1023 && pf_table_insert(t, 1023 + 1024, OWN) == 0 && pf_table_insert(t, 1023, OWN) == 1, "wrap");
        expect(pf_table_insert(t, 1023 + 1024, SHARE) == -1 && used(t) == 3, "wrap, found");
    }
    {   // ids with duplicates left out by a compare of the entries' bytes (the plot grid's strains): two names of one hash
        // are two entries, a name that comes twice is one
        const std::string names[4] = {"a", "b", "a", "b"};
        const uint64_t hash[4] = {42, 42, 42, 42};
        std::vector<unsigned long long> t(1024, 0);
        std::vector<uint32_t> id(1024, 0);
        int64_t at[4];
        for (uint32_t i = 0; i < 4; i++) {
            at[i] = pf_table_insert(t, hash[i], [&](uint64_t slot) { return names[id[slot]] == names[i]; });
            if (at[i] >= 0) id[at[i]] = i;
        }
        expect(at[0] == 42 && at[1] == 43 && at[2] == -1 && at[3] == -1 && id[42] == 0 && id[43] == 1, "duplicates by bytes");
    }
    {   // as many entries of one home slot as the load allows: every probe still ends at a free slot
        const uint64_t n = 255, cap = pf_table_room(n, 4);
        std::vector<uint64_t> t(cap, 0);
        bool ok = true;
        for (uint64_t i = 0; i < n; i++) ok = ok && pf_table_insert(t, 1000 + i * cap, OWN) == (int64_t)((1000 + i) % cap);
        expect(ok && used(t) == n, "a full run");
    }
    printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
