// out_file.h -- the file side of every device writer (ingest.hip: TSV; scaffold.hip: FASTA; pathtext.hip: .path and AGP;
// bgzf_deflate.hip: BGZF): one output file that cleans up after a failed call, and one way to put a block of bytes into it.
// Pure host code (tests/test_out_file_cpu.py compiles it on its own).
#pragma once

#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace mxg {

// n_parts byte ranges written to fd at consecutive offsets from `off` on, by that many threads (pwrite)
inline bool put_parallel(int fd, uint64_t off, const char *const *data, const size_t *len, uint32_t n_parts)
{
    std::vector<uint64_t> at(n_parts + 1, off);
    for (uint32_t t = 0; t < n_parts; ++t) at[t + 1] = at[t] + len[t];
    const uint64_t total = at[n_parts] - off;
    if (!total) return true;
    // (a shared mapping of the file filled by the workers was measured on the GPU boxes' /tmp and dropped: 1.2-1.35 s against
    // 0.8-0.9 s of pwrite for 1.9 GB of outputs -- write faults on a shared file mapping are no cheaper than the inode lock)
    std::atomic<bool> good{true};
    auto put = [&](uint32_t t) {
        size_t done = 0;
        while (done < len[t]) {
            const ssize_t wr = pwrite(fd, data[t] + done, len[t] - done, (off_t)(at[t] + done));
            if (wr <= 0) {
                good = false;
                return;
            }
            done += (size_t)wr;
        }
    };
    {
        std::vector<std::thread> th;
        for (uint32_t t = 1; t < n_parts; ++t) th.emplace_back(put, t);
        put(0);
        for (auto &x : th) x.join();
    }
    return good;
}

// how many threads put `bytes` bytes when the caller has `threads`: at most 16, each at least 1 MiB (0 for no bytes)
inline uint32_t put_parts(uint64_t bytes, uint32_t threads)
{
    return (uint32_t)std::min<uint64_t>(std::min(16u, std::max(1u, threads)), (bytes + (1u << 20) - 1) >> 20);
}

// A file that is removed again unless the call completes -- only a regular file this call created or truncated: a FIFO, a device,
// a process substitution, the NAME of a symbolic link to a regular file (/dev/stdout redirected into one) and "-" (stdout) are
// left alone.
struct OutFile {
    FILE *f = nullptr;
    std::string path;
    bool regular = false, removable = false, complete = false;
    bool open(const char *p)
    {
        path = p;
        if (path == "-") {  // (never regular, whatever the shell redirected it into: in order, at the descriptor's own position)
            f = stdout;
            return fflush(f) == 0;
        }
        f = fopen(p, "w+b");
        if (!f) return false;
        struct stat sb;
        regular = fstat(fileno(f), &sb) == 0 && S_ISREG(sb.st_mode);
        removable = regular && lstat(p, &sb) == 0 && S_ISREG(sb.st_mode);
        return true;
    }
    // The same for a call that adds to a file another call has written: what is there stays, *size is where the new bytes begin, and
    // the file is never removed (a failed call leaves what it found, and perhaps a part of its own behind it).  A file that does not
    // exist is created.
    bool open_append(const char *p, uint64_t *size)
    {
        path = p;
        *size = 0;
        f = fopen(p, "r+b");
        if (!f) f = fopen(p, "w+b");
        if (!f) return false;
        struct stat sb;
        if (fstat(fileno(f), &sb) != 0) return false;
        regular = S_ISREG(sb.st_mode);
        if (regular) *size = (uint64_t)sb.st_size;
        return true;
    }
    // A regular file takes the bytes at offset `off`, in put_parts(bytes, threads) parts side by side; anything else has no
    // offsets: it is written in order at the descriptor's own position, and `off` is not looked at.
    bool put(const char *src, uint64_t bytes, uint64_t off, uint32_t threads)
    {
        if (!bytes) return true;
        const int fd = fileno(f);
        if (!regular) {
            for (uint64_t done = 0; done < bytes;) {
                const ssize_t wr = write(fd, src + done, bytes - done);
                if (wr <= 0) return false;
                done += (uint64_t)wr;
            }
            return true;
        }
        const uint32_t T = put_parts(bytes, threads);
        const char *part[16];
        size_t len[16];
        for (uint32_t t = 0; t < T; ++t) {
            const uint64_t lo = bytes * t / T, hi = bytes * (t + 1) / T;
            part[t] = src + lo;
            len[t] = hi - lo;
        }
        return put_parallel(fd, off, part, len, T);
    }
    bool close()
    {
        if (!f) return true;
        const bool ok = f == stdout ? fflush(f) == 0 : fclose(f) == 0;
        f = nullptr;
        return ok;
    }
    ~OutFile()
    {
        (void)close();
        if (!complete && removable) (void)remove(path.c_str());
    }
};

}  // namespace mxg
