// volume_stream.h -- volumes read and inflated on host threads ahead of their consumer, handed out in list order.
//
// bin/AverageImage and bin/AverageVolumes take N volumes one after the other (the device adds them in file order).  Reading
// a compressed volume is a single-threaded inflate (0.1-0.2 s for 256^3 int16), so `threads` workers read the next files
// while the consumer's device work runs; at most `window` volumes (read or being read, not yet released) are held, so
// memory stays bounded whatever N is.  Thread counts come from usable_cpus() (affinity mask and cgroup quota), never from
// the machine's CPU count.
#pragma once

#include "../common/usable_cpus.h"
#include "frog_host.h"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace frog {

class VolumeStream {
public:
    struct Item {
        frog_volume_file *file = nullptr;
        frog_volume view{};
        int status = FROG_OK;
        double lo = 0, hi = 0;          // value range (VolumeTransform's default background is the minimum)
        double seconds = 0;             // read + inflate + range, on its worker
    };

    VolumeStream(const std::vector<std::string> &paths, int threads, size_t window)
        : paths_(paths), items_(paths.size()), ready_(paths.size(), 0)
    {
        window_ = std::max<size_t>(1, window);
        const int n = std::max(1, std::min<int>(threads, (int)paths.size()));
        for (int t = 0; t < n; t++) workers_.emplace_back([this] { work(); });
    }

    ~VolumeStream()
    {
        {
            std::lock_guard<std::mutex> l(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &w : workers_) w.join();
        for (auto &it : items_) if (it.file) frog_volume_free(it.file);
    }

    // blocks until volume i (taken in order 0, 1, ...) is read; `waited` receives the time spent blocked
    Item &get(size_t i, double *waited)
    {
        const auto t0 = std::chrono::steady_clock::now();
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return ready_[i] != 0; });
        if (waited) *waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return items_[i];
    }

    // frees volume i and lets a worker start on the next file beyond the window
    void release(size_t i)
    {
        {
            std::lock_guard<std::mutex> l(m_);
            if (items_[i].file) frog_volume_free(items_[i].file);
            items_[i].file = nullptr;
            released_++;
        }
        cv_.notify_all();
    }

    double read_seconds() const
    {
        double s = 0;
        for (const auto &it : items_) s += it.seconds;
        return s;
    }
    int threads() const { return (int)workers_.size(); }

private:
    void work()
    {
        for (;;) {
            size_t i;
            {
                std::unique_lock<std::mutex> l(m_);
                cv_.wait(l, [&] { return stop_ || (next_ < paths_.size() && next_ < released_ + window_); });
                if (stop_ || next_ >= paths_.size()) return;
                i = next_++;
            }
            Item it;
            const auto t0 = std::chrono::steady_clock::now();
            it.file = frog_volume_read(paths_[i].c_str(), &it.status);
            if (it.file) {
                frog_volume_view(it.file, &it.view);
                frog_volume_range(&it.view, &it.lo, &it.hi);
            } else if (it.status == FROG_OK) {
                it.status = FROG_E_IO;
            }
            it.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            {
                std::lock_guard<std::mutex> l(m_);
                items_[i] = it;
                ready_[i] = 1;
            }
            cv_.notify_all();
        }
    }

    std::vector<std::string> paths_;
    std::vector<Item> items_;
    std::vector<char> ready_;
    std::vector<std::thread> workers_;
    std::mutex m_;
    std::condition_variable cv_;
    size_t next_ = 0, released_ = 0, window_ = 1;
    bool stop_ = false;
};

// workers and window of a stream over n files: the usable CPUs less the consumer's own thread (16 at most), and one
// volume more in memory than there are workers
inline void volume_stream_shape(size_t n_files, int *threads, size_t *window)
{
    const int t = std::max(1, std::min<int>(usable_cpus() - 1, (int)std::min<size_t>(n_files, 16)));
    *threads = t;
    *window = std::max<size_t>(2, (size_t)t + 1);
}

} // namespace frog
