// What the library remembers about a structure, keyed by a tuple, at most `capacity` entries at a time.
//
// Host code only, plain C++17.  The rules every instance shares:
//   * an entry gets an arrival number when it is inserted, and the OLDEST ARRIVAL makes room for a new one,
//     however often it has been looked up since (the lifetime rule of include/gko_cdna4.h,
//     GKOC_TUNE_CSR_LONG_ROWS);
//   * the cache never destroys an entry and frees nothing: `insert` and `erase_if` hand what leaves to the
//     caller, who releases it AFTER dropping the lock that guards the cache (an entry owns device buffers, and
//     releasing those waits for the device);
//   * `count` is a relaxed atomic: the callers that only want to know whether anything is cached at all
//     (gkoc_free, every entry that writes an index array) pay one load and no lock.
// Everything but `count` is called with the caller's lock held; several caches may share one lock.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

namespace gkoc {

template <typename Key, typename Entry>
class structure_cache {
public:
    explicit structure_cache(size_t capacity) : capacity_(capacity) {}

    int count() const { return count_.load(std::memory_order_relaxed); }

    // the entry of `key`, or nullptr; valid until the entry leaves the cache
    Entry* find(const Key& key)
    {
        auto it = map_.find(key);
        return it == map_.end() ? nullptr : &it->second.entry;
    }

    // A new entry for `key`, which must not be cached.  In a full cache the oldest arrival goes to `dropped` first.
    Entry* insert(const Key& key, Entry entry, std::vector<Entry>* dropped)
    {
        if (map_.size() >= capacity_ && !map_.empty()) {
            auto oldest = map_.begin();
            for (auto it = map_.begin(); it != map_.end(); ++it) {
                if (it->second.arrival < oldest->second.arrival) oldest = it;
            }
            dropped->push_back(std::move(oldest->second.entry));
            map_.erase(oldest);
        }
        Entry* in = &map_.insert_or_assign(key, slot{std::move(entry), ++arrivals_}).first->second.entry;
        count_.store(int(map_.size()), std::memory_order_relaxed);
        return in;
    }

    // every entry with pred(key, entry) leaves the cache and goes to `dropped`
    template <typename Pred>
    void erase_if(Pred pred, std::vector<Entry>* dropped)
    {
        for (auto it = map_.begin(); it != map_.end();) {
            if (pred(it->first, static_cast<const Entry&>(it->second.entry))) {
                dropped->push_back(std::move(it->second.entry));
                it = map_.erase(it);
            } else {
                ++it;
            }
        }
        count_.store(int(map_.size()), std::memory_order_relaxed);
    }

    // fn(key, entry) for every entry, in key order
    template <typename Fn>
    void for_each(Fn fn) const
    {
        for (const auto& kv : map_) fn(kv.first, kv.second.entry);
    }

private:
    struct slot {
        Entry entry;
        uint64_t arrival;
    };
    std::map<Key, slot> map_;
    size_t capacity_;
    uint64_t arrivals_ = 0;
    std::atomic<int> count_{0};
};

}  // namespace gkoc
