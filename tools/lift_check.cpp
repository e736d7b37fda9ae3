// lift_check.cpp -- features lifted through a piece table (mxg_lift_prepare, mxg_lift_intervals, mxg_lift_bed) by the code of the
// device route run serially on the host (ntjoin_amd/csrc/lift.h, compose.h): the table's check and prefix, the index sorted by
// std::stable_sort with its running maximum, per feature the two bisections, the count, the status and the parts; for a BED file
// the line rules, the lifted lines and the unlifted ones.
//   lift_check intervals FILE [whole]
//       FILE holds numbers separated by white space: n_source and that many lengths; the table as n_records, then per record its
//       number of pieces and four numbers {record start end kind} per piece; the number of features and three numbers {record start
//       end} per feature
//       stdout: one line per feature: its status, its number of parts, then five numbers {s_record s_start s_end src_start reverse}
//       per part
//   lift_check bed FILE NAMES BED LIFTED UNLIFTED [whole]
//       FILE as above without the features; NAMES holds one name per line: the source records', then the table records'
//       (UNLIFTED "-": none); stdout: lines, skipped, features, the six status counts, parts, the bytes of either file
//   `whole`: MXG_LIFT_WHOLE_ONLY
//   exit status 0; 2: usage / unreadable file; 3: refused as MXG_EINVAL, 4: as MXG_ELIMIT (the reason on stderr)
// A stand-alone host program (c++ -std=c++17 -I include -I ntjoin_amd/csrc tools/lift_check.cpp); tests/test_lift_cpu.py builds it
// plainly and with AddressSanitizer + UndefinedBehaviorSanitizer.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>

#include "compose.h"
#include "lift.h"

using namespace mxg;

namespace {

struct Index {
    std::vector<uint32_t> src_len;
    std::vector<uint64_t> key, rmax;
    std::vector<LiftEntry> ent;
    uint64_t n_records = 0;
};

bool read_head(FILE *fh, Index &x, std::vector<mxg_seq_piece> &pieces, std::vector<uint64_t> &first)
{
    unsigned long long n = 0, m = 0;
    if (fscanf(fh, "%llu", &n) != 1) return false;
    x.src_len.resize(n);
    for (auto &v : x.src_len)
        if (fscanf(fh, "%u", &v) != 1) return false;
    if (fscanf(fh, "%llu", &n) != 1) return false;
    first.assign(1, 0);
    for (unsigned long long r = 0; r < n; ++r) {
        if (fscanf(fh, "%llu", &m) != 1) return false;
        for (unsigned long long j = 0; j < m; ++j) {
            mxg_seq_piece p;
            if (fscanf(fh, "%u %u %u %u", &p.record, &p.start, &p.end, &p.kind) != 4) return false;
            pieces.push_back(p);
        }
        first.push_back(pieces.size());
    }
    x.n_records = n;
    return true;
}

int refuse(int rc, const std::string &msg)
{
    fprintf(stderr, "%s\n", msg.c_str());
    return rc == MXG_ELIMIT ? 4 : 3;
}

// mxg_lift_prepare on the host
int prepare(Index &x, const std::vector<mxg_seq_piece> &pieces, const std::vector<uint64_t> &first, std::string &msg)
{
    if (x.src_len.size() >= LFT_MAX) {
        msg = "too many source records";
        return MXG_ELIMIT;
    }
    CmpTable tab;
    const int rc = cmp_table("table", pieces.data(), first.data(), x.n_records, x.src_len.size(), x.src_len.data(), tab, msg);
    if (rc != MXG_OK) return rc;
    std::vector<uint32_t> seq;
    for (uint32_t j = 0; j < pieces.size(); ++j)
        if (pieces[j].kind != MXG_PIECE_GAP) seq.push_back(j);
    std::stable_sort(seq.begin(), seq.end(), [&](uint32_t i, uint32_t j) {
        return lift_key(pieces[i].record, pieces[i].start) < lift_key(pieces[j].record, pieces[j].start);
    });
    uint64_t run = 0;
    for (uint32_t j : seq) {
        const mxg_seq_piece &p = pieces[j];
        x.key.push_back(lift_key(p.record, p.start));
        x.ent.push_back(LiftEntry{p.start, p.end, tab.rec[j] | (p.kind == MXG_PIECE_REV ? LFT_REV : 0u), tab.pre[j]});
        run = std::max(run, lift_key(p.record, p.end));
        x.rmax.push_back(run);
    }
    return MXG_OK;
}

struct Lifted {
    std::vector<uint32_t> status;
    std::vector<uint64_t> part_first{0};
    std::vector<LiftPart> parts;
};

// mxg_lift_intervals on the host: count first, refuse, then emit
int lift(const Index &x, const std::vector<uint32_t> &rec, const std::vector<uint32_t> &a, const std::vector<uint32_t> &b, bool whole_only, Lifted &out,
         std::string &msg)
{
    const size_t n = rec.size();
    const uint32_t m = (uint32_t)x.key.size();
    if (n >= LFT_MAX) {
        msg = "too many features";
        return MXG_ELIMIT;
    }
    std::vector<uint32_t> lo(n, 0), hi(n, 0);
    std::vector<uint64_t> cnt(n, 0);
    out.status.assign(n, MXG_LIFT_INVALID);
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!lift_valid(rec[i], a[i], b[i], x.src_len.size(), x.src_len.data())) continue;
        lift_range(x.key.data(), x.rmax.data(), m, rec[i], a[i], b[i], lo[i], hi[i]);
        out.status[i] = lift_count(x.ent.data(), lo[i], hi[i], a[i], b[i], cnt[i]);
        if (whole_only && out.status[i] != MXG_LIFT_WHOLE) cnt[i] = 0;
        total += cnt[i];
    }
    if (total >= LFT_MAX) {
        msg = "the features have " + std::to_string(total) + " parts (fewer than 2^31)";
        return MXG_ELIMIT;
    }
    out.parts.reserve(total);
    for (size_t i = 0; i < n; ++i) {
        if (cnt[i])
            for (uint32_t j = lo[i]; j < hi[i]; ++j)
                if (x.ent[j].end > a[i]) out.parts.push_back(lift_part(x.ent[j], a[i], b[i]));
        out.part_first.push_back(out.parts.size());
    }
    return MXG_OK;
}

bool read_file(const char *path, std::string &out)
{
    FILE *fh = fopen(path, "rb");
    if (!fh) return false;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, fh)) > 0) out.append(buf, got);
    fclose(fh);
    return true;
}

std::vector<std::string> split_lines(const std::string &t)
{
    std::vector<std::string> out;
    for (size_t at = 0; at < t.size();) {
        size_t e = t.find('\n', at);
        if (e == std::string::npos) e = t.size();
        out.push_back(t.substr(at, e - at));
        at = e + 1;
    }
    return out;
}

bool write_file(const char *path, const std::string &t)
{
    FILE *fh = fopen(path, "wb");
    if (!fh) return false;
    const bool ok = fwrite(t.data(), 1, t.size(), fh) == t.size();
    return fclose(fh) == 0 && ok;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    const bool bed = mode == "bed";
    if (!bed && mode != "intervals") return 2;
    if (bed ? (argc != 7 && argc != 8) : (argc != 3 && argc != 4)) return 2;
    const char *last = argv[argc - 1];
    const bool whole_only = (bed ? argc == 8 : argc == 4) && strcmp(last, "whole") == 0;
    if ((bed ? argc == 8 : argc == 4) && !whole_only) return 2;
    FILE *fh = fopen(argv[2], "r");
    if (!fh) return 2;
    Index x;
    std::vector<mxg_seq_piece> pieces;
    std::vector<uint64_t> first;
    std::vector<uint32_t> rec, a, b;
    bool ok = read_head(fh, x, pieces, first);
    if (ok && !bed) {
        unsigned long long n = 0;
        ok = fscanf(fh, "%llu", &n) == 1;
        for (unsigned long long i = 0; ok && i < n; ++i) {
            uint32_t r, s, e;
            ok = fscanf(fh, "%u %u %u", &r, &s, &e) == 3;
            rec.push_back(r), a.push_back(s), b.push_back(e);
        }
    }
    fclose(fh);
    if (!ok) return 2;
    std::string msg;
    int rc = prepare(x, pieces, first, msg);
    if (rc != MXG_OK) return refuse(rc, msg);
    Lifted L;
    if (!bed) {
        if ((rc = lift(x, rec, a, b, whole_only, L, msg)) != MXG_OK) return refuse(rc, msg);
        for (size_t i = 0; i < rec.size(); ++i) {
            printf("%u %llu", L.status[i], (unsigned long long)(L.part_first[i + 1] - L.part_first[i]));
            for (uint64_t g = L.part_first[i]; g < L.part_first[i + 1]; ++g) {
                const LiftPart &p = L.parts[g];
                printf(" %u %u %u %u %u", p.s_record, p.s_start, p.s_end, p.src_start, p.reverse);
            }
            printf("\n");
        }
        return 0;
    }
    // ---- a BED file
    std::string names_text, text;
    if (!read_file(argv[3], names_text) || !read_file(argv[4], text)) return 2;
    const std::vector<std::string> names = split_lines(names_text);
    const size_t n_source = x.src_len.size();
    if (names.size() != n_source + x.n_records) return 2;
    std::unordered_map<std::string, uint32_t> by_name;
    for (size_t r = 0; r < n_source; ++r) by_name.emplace(names[r], (uint32_t)r);  // (the first record of a name wins)
    unsigned long long lines = 0, skipped = 0, n_status[6] = {0, 0, 0, 0, 0, 0};
    std::vector<uint64_t> line_off, line_len;
    std::vector<BedLine> parsed;
    std::vector<uint8_t> unknown;
    for (uint64_t at = 0; at < text.size();) {
        const void *nl = memchr(text.data() + at, '\n', text.size() - at);
        const uint64_t end = nl ? (uint64_t)(static_cast<const char *>(nl) - text.data()) : text.size();
        const char *line = text.data() + at;
        ++lines;
        if (bed_skipped(line, end - at)) {
            ++skipped;
        } else {
            const BedLine bl = bed_parse(line, end - at);
            uint32_t r = LFT_NONE, s = 0, e = 0;
            bool unk = false;
            if (bl.ok) {
                s = bl.a, e = bl.b;
                const auto it = by_name.find(std::string(line, bl.name_len));
                if (it != by_name.end()) r = it->second;
                else if (s < e) unk = true;
            }
            rec.push_back(r), a.push_back(s), b.push_back(e);
            unknown.push_back(unk);
            parsed.push_back(bl);
            line_off.push_back(at), line_len.push_back(bed_line_end(line, end - at));
        }
        at = nl ? end + 1 : text.size();
    }
    if ((rc = lift(x, rec, a, b, whole_only, L, msg)) != MXG_OK) return refuse(rc, msg);
    std::string lifted, unlifted;
    for (size_t i = 0; i < rec.size(); ++i) {
        if (unknown[i]) L.status[i] = MXG_LIFT_UNKNOWN;
        ++n_status[L.status[i]];
        const char *line = text.data() + line_off[i];
        const BedLine &bl = parsed[i];
        for (uint64_t g = L.part_first[i]; g < L.part_first[i + 1]; ++g) {
            const LiftPart &p = L.parts[g];
            lifted += names[n_source + p.s_record] + "\t" + std::to_string(p.s_start) + "\t" + std::to_string(p.s_end);
            if (bl.rest_off) {
                lifted += '\t';
                const size_t at = lifted.size();
                lifted.append(line + bl.rest_off, bl.rest_len);
                if (bl.strand_off && p.reverse) lifted[at + (bl.strand_off - bl.rest_off)] = lift_flip(line[bl.strand_off]);
            }
            lifted += '\n';
        }
        if (L.status[i] != MXG_LIFT_WHOLE) {
            unlifted += std::string("#") + lift_reason(L.status[i]) + "\n";
            unlifted.append(line, line_len[i]);
            unlifted += '\n';
        }
    }
    if (!write_file(argv[5], lifted)) return 2;
    const bool with_un = strcmp(argv[6], "-") != 0;
    if (with_un && !write_file(argv[6], unlifted)) return 2;
    printf("%llu %llu %zu %llu %llu %llu %llu %llu %llu %zu %zu %zu\n", lines, skipped, rec.size(), n_status[0], n_status[1], n_status[2], n_status[3],
           n_status[4], n_status[5], L.parts.size(), lifted.size(), with_un ? unlifted.size() : (size_t)0);
    return 0;
}
