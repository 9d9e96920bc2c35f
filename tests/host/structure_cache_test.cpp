// Host test of ginkgo_amd/csrc/structure_cache.hpp, the mechanism of the two CSR structure caches
// (csr_structure.hip).  Built and run by tests/test_structure_cache_cpu.py:
//   g++ -std=c++17 -pthread -I ginkgo_amd/csrc tests/host/structure_cache_test.cpp
// Entries carry an integer id, so every entry that was ever inserted can be accounted for.
#include "structure_cache.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <random>
#include <thread>
#include <tuple>

using key_t_ = std::tuple<int, int64_t>;
struct entry {
    int id;
};
using cache_t = gkoc::structure_cache<key_t_, entry>;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

// The lock that guards a cache, as the library's callers hold it - and it knows its holder, so that a release step
// can tell "this thread still holds it" (the bug) from "another thread holds it right now" (contention).
class cache_lock {
public:
    void lock()
    {
        m_.lock();
        holder_.store(std::this_thread::get_id());
    }
    bool try_lock()
    {
        if (!m_.try_lock()) return false;
        holder_.store(std::this_thread::get_id());
        return true;
    }
    void unlock()
    {
        holder_.store(std::thread::id());
        m_.unlock();
    }
    bool held_by_me() const { return holder_.load() == std::this_thread::get_id(); }

private:
    std::mutex m_;
    std::atomic<std::thread::id> holder_{};
};

std::vector<int> ids_of(const std::vector<entry>& v)
{
    std::vector<int> ids;
    for (const entry& e : v) ids.push_back(e.id);
    return ids;
}

// capacity 8, ten keys: the two oldest ARRIVALS make room, in arrival order, however often they were looked up
void test_oldest_arrival_makes_room()
{
    constexpr int C = 8;
    cache_t cache(C);
    cache_lock lock;
    std::vector<entry> dropped;
    CHECK(cache.count() == 0);
    {
        std::lock_guard<cache_lock> g(lock);
        for (int k = 0; k < C; ++k) {
            CHECK(cache.find(key_t_{0, k}) == nullptr);
            CHECK(cache.insert(key_t_{0, k}, entry{100 + k}, &dropped)->id == 100 + k);
        }
        CHECK(dropped.empty() && cache.count() == C);
        for (int round = 0; round < 50; ++round) {
            CHECK(cache.find(key_t_{0, 0})->id == 100 && cache.find(key_t_{0, 1})->id == 101);
        }
        cache.insert(key_t_{0, C}, entry{100 + C}, &dropped);
        CHECK(ids_of(dropped) == std::vector<int>{100});
        for (int round = 0; round < 50; ++round) CHECK(cache.find(key_t_{0, 1})->id == 101);
        cache.insert(key_t_{0, C + 1}, entry{100 + C + 1}, &dropped);
        CHECK((ids_of(dropped) == std::vector<int>{100, 101}));
        CHECK(cache.count() == C);
        CHECK(cache.find(key_t_{0, 0}) == nullptr && cache.find(key_t_{0, 1}) == nullptr);
        for (int k = 2; k < C + 2; ++k) CHECK(cache.find(key_t_{0, k})->id == 100 + k);
    }
    // the release step: the lock is free again
    CHECK(lock.try_lock());
    lock.unlock();
}

// erase_if hands back exactly the matching entries, and the count follows
void test_erase_if()
{
    cache_t cache(8);
    cache_lock lock;
    std::vector<entry> dropped, gone;
    {
        std::lock_guard<cache_lock> g(lock);
        cache.erase_if([](const key_t_&, const entry&) { return true; }, &gone);
        CHECK(gone.empty() && cache.count() == 0);
        for (int k = 0; k < 8; ++k) cache.insert(key_t_{k % 2, k}, entry{k}, &dropped);
        CHECK(dropped.empty() && cache.count() == 8);
        cache.erase_if([](const key_t_& k, const entry& e) { return std::get<0>(k) == 1 && e.id != 7; }, &gone);
        std::vector<int> ids = ids_of(gone);
        std::sort(ids.begin(), ids.end());
        CHECK((ids == std::vector<int>{1, 3, 5}));
        CHECK(cache.count() == 5);
        for (int k : {0, 2, 4, 6, 7}) CHECK(cache.find(key_t_{k % 2, k})->id == k);
        for (int k : {1, 3, 5}) CHECK(cache.find(key_t_{k % 2, k}) == nullptr);
        gone.clear();
        cache.erase_if([](const key_t_&, const entry&) { return true; }, &gone);
        CHECK(gone.size() == 5 && cache.count() == 0);
    }
    CHECK(lock.try_lock());
    lock.unlock();
}

// Four threads, mixed calls, the callers' discipline: look up and insert under the lock, release what was handed
// back after unlocking.  Every entry ever inserted is handed back exactly once or is still cached at the end.
void test_threads()
{
    constexpr int THREADS = 4, CALLS = 4000, KEYS = 300, C = 64;
    cache_t cache(C);
    cache_lock lock;
    std::atomic<int> next_id{0};
    std::atomic<long> uncontended{0};
    std::vector<std::vector<int>> inserted(THREADS), returned(THREADS);

    auto work = [&](int t) {
        std::mt19937 rng(1234 + t);
        // The release step takes the cache's lock itself, as the library's does for its graveyard.  try_lock proves
        // that the entries were handed back outside the lock; where it fails, ANOTHER thread must be the holder
        // (this thread holding it would block below for ever), and the step waits for it.
        auto release = [&](std::vector<entry>& dropped) {
            CHECK(!lock.held_by_me());
            if (lock.try_lock()) {
                ++uncontended;
            } else {
                lock.lock();
            }
            CHECK(cache.count() >= 0 && cache.count() <= C);
            lock.unlock();
            for (const entry& e : dropped) returned[t].push_back(e.id);
            dropped.clear();
        };
        std::vector<entry> dropped;
        for (int i = 0; i < CALLS; ++i) {
            const key_t_ key{int(rng() % 3), int64_t(rng() % (KEYS / 3))};
            const unsigned what = rng() % 8;
            {
                std::lock_guard<cache_lock> g(lock);
                if (what < 4) {
                    if (cache.find(key) == nullptr) {
                        const int id = next_id++;
                        inserted[t].push_back(id);
                        CHECK(cache.insert(key, entry{id}, &dropped)->id == id);
                    }
                } else if (what < 7) {
                    const entry* e = cache.find(key);
                    CHECK(e == nullptr || (e->id >= 0 && e->id < next_id.load()));
                } else {
                    const int64_t r = int64_t(rng() % 16);
                    cache.erase_if([&](const key_t_& k, const entry&) { return std::get<1>(k) % 16 == r; }, &dropped);
                }
            }
            release(dropped);
        }
    };
    std::vector<std::thread> threads;
    for (int t = 0; t < THREADS; ++t) threads.emplace_back(work, t);
    for (auto& th : threads) th.join();

    std::vector<entry> rest;
    {
        std::lock_guard<cache_lock> g(lock);
        CHECK(cache.count() <= C);
        const int left = cache.count();
        cache.erase_if([](const key_t_&, const entry&) { return true; }, &rest);
        CHECK(int(rest.size()) == left && cache.count() == 0);
    }
    std::vector<int> in, out = ids_of(rest);
    for (int t = 0; t < THREADS; ++t) {
        in.insert(in.end(), inserted[t].begin(), inserted[t].end());
        out.insert(out.end(), returned[t].begin(), returned[t].end());
    }
    std::sort(in.begin(), in.end());
    std::sort(out.begin(), out.end());
    CHECK(int(in.size()) == next_id.load());
    CHECK(std::adjacent_find(out.begin(), out.end()) == out.end());      // nothing handed back twice
    CHECK(in == out);                                                    // nothing lost
    CHECK(uncontended.load() > 0);
    std::printf("threads: %d entries inserted, %zu still cached at the end, %ld of %d release steps found the lock "
                "free at once\n",
                next_id.load(), rest.size(), uncontended.load(), THREADS * CALLS);
}

int main()
{
    test_oldest_arrival_makes_room();
    test_erase_if();
    test_threads();
    std::printf("structure_cache_test OK\n");
    return 0;
}
