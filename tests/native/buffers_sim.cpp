// tetrex_amd/csrc/txq_buffers.hpp on a counting allocator (tests/test_buffers_cpu.py builds this with the address and
// undefined-behaviour sanitizers): every request, free and destroyed handle is recorded, the n-th allocation can be told to
// fail, and each case below ends by checking that nothing is live and nothing was freed twice.
#include "../../tetrex_amd/csrc/txq_buffers.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

using namespace txq;

static int g_failures = 0;
#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++g_failures;                                                     \
        }                                                                     \
    } while (0)

// Sizes are made up (up to hundreds of MiB): a block is 16 real bytes, the request is what is recorded.
struct Mem {
    static inline std::vector<size_t> requests;
    static inline std::vector<std::string>* log = nullptr;  // "free" is appended here where a case watches the order of events
    static inline std::set<void*> live;
    static inline int frees = 0, double_frees = 0, fail_at = 0;  // fail_at: the allocation (counted from 1) that fails; 0: none
    static int alloc(void** p, size_t bytes) {
        requests.push_back(bytes);
        if (fail_at && (int)requests.size() == fail_at) return 2;  // (an error code of the policy's own)
        *p = std::malloc(16);
        live.insert(*p);
        return 0;
    }
    static void free(void* p) {
        ++frees;
        if (log) log->push_back("free");
        if (!live.erase(p)) { ++double_frees; return; }
        std::free(p);
    }
    static void start() {
        CHECK(live.empty());
        requests.clear();
        frees = double_frees = fail_at = 0;
        log = nullptr;
    }
    static void end(const char* what) {
        CHECK(live.empty());
        CHECK(double_frees == 0);
        std::printf("%s: %zu allocations, %d frees, %zu live, %d double frees\n", what, requests.size(), frees, live.size(), double_frees);
    }
};
using Buf = Buffer<unsigned char, Mem>;
using Words = Buffer<unsigned long long, Mem>;
constexpr size_t MiB = (size_t)1 << 20;

static void keeps_what_is_large_enough() {
    Mem::start();
    {
        Buf b;
        CHECK(b.get() == nullptr && b.bytes() == 0 && !b);
        CHECK(b.reserve(exactly(1000), free_now()) == 0);
        unsigned char* p = b.get();
        CHECK(p && b.bytes() == 1000);
        int hooks = 0;
        auto hook = [&](auto&&) { ++hooks; };
        CHECK(b.reserve(exactly(1000), hook) == 0 && b.get() == p);
        CHECK(b.reserve(exactly(1), hook) == 0 && b.get() == p);
        CHECK(b.reserve(half_more(600, 0), hook) == 0 && b.get() == p);  // (900 wanted, but 600 needed: it stays)
        CHECK(b.bytes() == 1000 && hooks == 0 && Mem::requests.size() == 1 && Mem::frees == 0);
    }
    CHECK(Mem::frees == 1);
    Mem::end("keeps");
}

static void asks_for_what_the_rule_says() {
    Mem::start();
    {
        const Grow rules[] = {exactly(12345),          exactly(12346),           half_more(100, MiB),      half_more(MiB, MiB),
                              half_more(10 * MiB, 16 * MiB), half_more(16 * MiB, 16 * MiB), half_more(40 * MiB, 64 * MiB), half_more(100 * MiB + 1, 64 * MiB)};
        const size_t want[] = {12345, 12346, MiB, MiB + MiB / 2, 16 * MiB, 24 * MiB, 64 * MiB, 100 * MiB + 1 + (100 * MiB + 1) / 2};
        for (size_t i = 0; i < 8; ++i) {  // from nothing, and from one byte less than is needed
            Buf b, c;
            CHECK(rules[i].want == want[i]);
            CHECK(b.reserve(rules[i], free_now()) == 0);
            CHECK(b.bytes() == want[i] && Mem::requests.back() == want[i]);
            CHECK(c.reserve(exactly(rules[i].need - 1), free_now()) == 0 && c.reserve(rules[i], free_now()) == 0);
            CHECK(c.bytes() == want[i] && Mem::requests.back() == want[i]);
        }
        CHECK(Mem::requests.size() == 24 && Mem::frees == 24);
        // the staging masks of a stage: the need has a floor of 16 MiB, then half as much again
        CHECK(half_more(std::max<size_t>(5, 16 * MiB), MiB).want == 24 * MiB);
    }
    Mem::end("growth");
}

static void outgrown_rules() {
    Mem::start();
    std::vector<std::string> log;
    {
        Buf b;
        CHECK(b.reserve(exactly(10), free_now()) == 0);
        Mem::log = &log;
        // freed after a wait (the device-wide wait and the wait for a named event are both this, with another wait)
        CHECK(b.reserve(exactly(20), free_after([&] { log.push_back("device wait"); })) == 0);
        CHECK(b.reserve(exactly(30), free_after([&] { log.push_back("event wait"); })) == 0);
        CHECK((log == std::vector<std::string>{"device wait", "free", "event wait", "free"}));
        // freed at once
        CHECK(b.reserve(exactly(40), free_now()) == 0);
        CHECK(log.size() == 5 && log.back() == "free");
        // any hook of the call site's own: once, before the free
        CHECK(b.reserve(exactly(50), [&](auto&& old) { CHECK(old.bytes() == 40); log.push_back("hook"); }) == 0);
        CHECK(log.size() == 7 && log[5] == "hook" && log[6] == "free");
        // retired: nothing is freed until the list dies
        {
            std::vector<Buffer<void, Mem>> retired;
            unsigned char* old = b.get();
            CHECK(b.reserve(exactly(60), retire_to(retired)) == 0);
            CHECK(b.reserve(half_more(61, 0), retire_to(retired)) == 0);
            CHECK(log.size() == 7 && retired.size() == 2 && retired[0].get() == old && retired[0].bytes() == 50 && retired[1].bytes() == 60);
            CHECK(b.bytes() == 91 && Mem::live.size() == 3);
        }
        CHECK(log.size() == 9 && Mem::live.size() == 1);
        // an empty buffer has nothing outgrown: no hook
        Buf fresh;
        CHECK(fresh.reserve(exactly(8), [&](auto&&) { log.push_back("never"); }) == 0 && log.size() == 9);
    }
    Mem::end("outgrown");
}

static void failed_allocation() {
    Mem::start();
    {
        Buf b;
        Mem::fail_at = 1;
        CHECK(b.reserve(exactly(100), free_now()) == 2);
        CHECK(b.get() == nullptr && b.bytes() == 0);
        CHECK(b.reserve(exactly(100), free_now()) == 0 && b.get() && b.bytes() == 100);
        Mem::fail_at = 3;  // growing fails: the old block is gone (its rule ran), no stale capacity stays behind
        int hooks = 0;
        CHECK(b.reserve(half_more(200, 0), [&](auto&&) { ++hooks; }) == 2);
        CHECK(hooks == 1 && b.get() == nullptr && b.bytes() == 0 && Mem::live.empty());
        CHECK(b.reserve(exactly(50), [&](auto&&) { ++hooks; }) == 0 && hooks == 1 && b.bytes() == 50);
    }
    Mem::end("failure");
}

static void moves() {
    Mem::start();
    {
        Buf a, b;
        CHECK(a.reserve(exactly(10), free_now()) == 0 && b.reserve(exactly(20), free_now()) == 0);
        unsigned char* pa = a.get();
        Buf c(std::move(a));
        CHECK(!a && a.bytes() == 0 && c.get() == pa && c.bytes() == 10 && Mem::frees == 0);
        b = std::move(c);  // the target's old block is freed, once
        CHECK(!c && c.bytes() == 0 && b.get() == pa && b.bytes() == 10 && Mem::frees == 1);
        Buf& self = b;
        b = std::move(self);
        CHECK(b.get() == pa && Mem::frees == 1);
        Buffer<void, Mem> v(std::move(b));  // any element type goes onto a retire list
        CHECK(!b && v.get() == pa && v.bytes() == 10);
        a = Buf{};
        CHECK(Mem::frees == 1);
        b.reset();
        CHECK(Mem::frees == 1);
    }
    CHECK(Mem::frees == 2);
    Mem::end("moves");
}

// events and streams
struct Kind {
    static inline std::vector<int*> destroyed;
    static void destroy(int* h) { destroyed.push_back(h); }
};
using Ev = Handle<int*, Kind>;

static void handles() {
    int x = 0, y = 0;
    Kind::destroyed.clear();
    {
        Ev a, b;
        CHECK(!a && a.get() == nullptr);
        a.reset(&x);
        CHECK(a && a.get() == &x);
        Ev c(std::move(a));
        CHECK(!a && c.get() == &x && Kind::destroyed.empty());
        b.reset(&y);
        b = std::move(c);
        CHECK(!c && b.get() == &x && (Kind::destroyed == std::vector<int*>{&y}));
        a.reset();
        CHECK(Kind::destroyed.size() == 1);
    }
    CHECK((Kind::destroyed == std::vector<int*>{&y, &x}));
    std::printf("handles: %zu destroyed\n", Kind::destroyed.size());
}

// A session and an index's cache as libtxq shapes them (txq_internal.hpp SessionBuffers, SessionCache, Session).
struct Chunk { unsigned long long* p; size_t cap; };
struct Staging { Buf blob, aux; Words masks; Ev done; };
struct SessionBuffers { Staging set[2]; Ev upload, side; Words final_masks; };
struct Cache : SessionBuffers {
    std::vector<Chunk> chunks;
    bool in_use = false;
    ~Cache() { free_chunks<Mem>(chunks); }
};
struct MockSession : SessionBuffers {
    Cache* cache = nullptr;  // null: this session did not get the cache
    std::vector<Chunk> chunks;
    std::vector<Buffer<void, Mem>> retired;
    explicit MockSession(Cache& c) {
        if (c.in_use) return;
        c.in_use = true;
        cache = &c;
        static_cast<SessionBuffers&>(*this) = std::move(static_cast<SessionBuffers&>(c));
        chunks.swap(c.chunks);
    }
    void stage(size_t i, size_t bytes) {
        CHECK(set[i].blob.reserve(half_more(bytes, MiB), retire_to(retired)) == 0);
        CHECK(set[i].masks.reserve(half_more(std::max(bytes, 16 * MiB), MiB), retire_to(retired)) == 0);
        void* p = nullptr;
        CHECK(Mem::alloc(&p, bytes) == 0);
        chunks.push_back(Chunk{(unsigned long long*)p, bytes / 8});
    }
    ~MockSession() {
        retired.clear();
        if (cache) {
            cache->chunks.swap(chunks);
            static_cast<SessionBuffers&>(*cache) = std::move(static_cast<SessionBuffers&>(*this));
            cache->in_use = false;
        }
        free_chunks<Mem>(chunks);
    }
};

static void session_round_trip() {
    Mem::start();
    Kind::destroyed.clear();
    int ev[4];
    {
        Cache cache;
        {
            MockSession a(cache), b(cache);
            CHECK(a.cache == &cache && b.cache == nullptr);
            a.set[0].done.reset(&ev[0]);
            a.upload.reset(&ev[1]);
            b.set[0].done.reset(&ev[2]);
            a.stage(0, 2 * MiB);
            a.stage(1, 3 * MiB);
            b.stage(0, MiB);
            unsigned char* first = a.set[0].blob.get();
            a.stage(0, 40 * MiB);  // outgrows set 0's blob and masks: both are retired, not freed
            CHECK(a.retired.size() == 2 && a.retired[0].get() == first && Mem::frees == 0);
            CHECK(a.set[0].blob.bytes() == 60 * MiB && a.set[0].masks.bytes() == 60 * MiB);
            CHECK(a.final_masks.reserve(half_more(100, MiB), free_now()) == 0);
            CHECK(b.final_masks.reserve(half_more(100, MiB), free_now()) == 0 && a.final_masks.get() != b.final_masks.get());
        }
        // b freed all it made (2 buffers, 1 chunk, its final masks, its event); a freed what it retired and handed the rest back
        CHECK(!cache.in_use && cache.chunks.size() == 3 && cache.set[0].blob.bytes() == 60 * MiB && cache.set[1].blob.bytes() == 3 * MiB + 3 * MiB / 2);
        CHECK(cache.set[0].done.get() == &ev[0] && cache.upload.get() == &ev[1] && cache.final_masks.bytes() == MiB);
        CHECK(Mem::frees == 4 + 2 && (Kind::destroyed == std::vector<int*>{&ev[2]}));
        {
            MockSession c(cache);  // the next session adopts it all: nothing is allocated for a stage that fits
            const size_t before = Mem::requests.size();
            CHECK(c.cache == &cache && c.chunks.size() == 3 && !cache.set[0].blob && cache.chunks.empty());
            CHECK(c.set[0].blob.reserve(half_more(50 * MiB, MiB), retire_to(c.retired)) == 0 && c.retired.empty() && Mem::requests.size() == before);
        }
    }
    CHECK(Kind::destroyed.size() == 3);
    Mem::end("session");
}

int main() {
    keeps_what_is_large_enough();
    asks_for_what_the_rule_says();
    outgrown_rules();
    failed_allocation();
    moves();
    handles();
    session_round_trip();
    std::printf("%s\n", g_failures ? "FAILED" : "ok");
    return g_failures ? 1 : 0;
}
