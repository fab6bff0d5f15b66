// Host half of the BUS writer: ec numbering and the file writers (bus_host.hpp). No HIP here.
#include "bus_host.hpp"

#include <sys/stat.h>

#include <algorithm>
#include <cerrno>

namespace pa {
namespace bus {

namespace {

struct Span {
    const uint32_t* p;
    uint64_t n;
};

// lexicographic order of id lists: {1,5} < {1,5,7} < {2,3}
bool span_less(const Span& a, const Span& b) { return std::lexicographical_compare(a.p, a.p + a.n, b.p, b.p + b.n); }
bool span_equal(const Span& a, const Span& b) { return a.n == b.n && std::equal(a.p, a.p + a.n, b.p); }

char* put_u64(char* p, uint64_t v) {   // decimal digits of v at p; returns the end
    char tmp[20];
    int n = 0;
    do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) *p++ = tmp[--n];
    return p;
}

void put_le32(std::string& s, uint32_t v) {
    for (int j = 0; j < 4; ++j) s.push_back((char)((v >> (8 * j)) & 0xFF));
}
void put_le64(std::string& s, uint64_t v) {
    for (int j = 0; j < 8; ++j) s.push_back((char)((v >> (8 * j)) & 0xFF));
}

int write_all(const std::string& path, const std::string& text) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return fail(PA_ERR_IO, "cannot create %s: %s", path.c_str(), strerror(errno));
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    if (fclose(f) != 0 || !ok) return fail(PA_ERR_IO, "cannot write %s", path.c_str());
    return PA_OK;
}

}  // namespace

int class_ecs(uint32_t T, const uint64_t* ec_offset, const uint32_t* ec_ids, uint32_t num_classes, std::vector<uint32_t>& class_ec, uint32_t* M) {
    class_ec.assign(num_classes, CLASS_EC_NONE);
    uint64_t m = 0;
    for (uint32_t c = 0; c < num_classes; ++c) {
        const uint64_t a = ec_offset[c], len = ec_offset[c + 1] - a;
        if (len == 1) {
            if (ec_ids[a] < T) class_ec[c] = ec_ids[a];
        } else if (len >= 2) {
            if ((uint64_t)T + m + 1 > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "more than 2^31-1 equivalence classes");
            class_ec[c] = (uint32_t)(T + m);
            ++m;
        }
    }
    *M = (uint32_t)m;
    return PA_OK;
}

int assign_ecs(uint32_t T, const uint64_t* ec_offset, const uint32_t* ec_ids, uint32_t num_classes, const uint64_t* list_off, const uint32_t* list_ids,
               uint64_t n_lists, EcTable& table, std::vector<int32_t>& list_ec) {
    std::vector<uint32_t> class_ec;
    uint32_t M = 0;
    int e = class_ecs(T, ec_offset, ec_ids, num_classes, class_ec, &M);
    if (e != PA_OK) return e;
    // the index classes of two ids or more, ordered by content (then class id: of two classes of equal content the first is met)
    std::vector<uint32_t> multi;
    multi.reserve(M);
    for (uint32_t c = 0; c < num_classes; ++c)
        if (class_ec[c] != CLASS_EC_NONE && ec_offset[c + 1] - ec_offset[c] >= 2) multi.push_back(c);
    auto class_span = [&](uint32_t c) { return Span{ec_ids + ec_offset[c], ec_offset[c + 1] - ec_offset[c]}; };
    auto list_span = [&](uint64_t l) { return Span{list_ids + list_off[l], list_off[l + 1] - list_off[l]}; };
    std::sort(multi.begin(), multi.end(), [&](uint32_t a, uint32_t b) {
        const Span sa = class_span(a), sb = class_span(b);
        if (span_less(sa, sb)) return true;
        if (span_less(sb, sa)) return false;
        return a < b;
    });
    // the lists by content; equal ones are neighbours
    std::vector<uint64_t> order(n_lists);
    for (uint64_t l = 0; l < n_lists; ++l) order[l] = l;
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        const Span sa = list_span(a), sb = list_span(b);
        if (span_less(sa, sb)) return true;
        if (span_less(sb, sa)) return false;
        return a < b;
    });
    list_ec.assign(n_lists, -1);
    std::vector<uint64_t> novel;   // one list of every novel content, in lexicographic order
    for (uint64_t i = 0; i < n_lists; ++i) {
        const uint64_t l = order[i];
        const Span s = list_span(l);
        if (i > 0 && span_equal(s, list_span(order[i - 1]))) {
            list_ec[l] = list_ec[order[i - 1]];
            continue;
        }
        const auto it = std::lower_bound(multi.begin(), multi.end(), s, [&](uint32_t c, const Span& x) { return span_less(class_span(c), x); });
        if (it != multi.end() && span_equal(class_span(*it), s)) {
            list_ec[l] = (int32_t)class_ec[*it];
            continue;
        }
        if ((uint64_t)T + M + novel.size() + 1 > 0x7FFFFFFFull) return fail(PA_ERR_UNSUPPORTED, "more than 2^31-1 equivalence classes");
        list_ec[l] = (int32_t)((uint64_t)T + M + novel.size());
        novel.push_back(l);
    }
    // the table of every ec: singletons, index classes in class-id order, novel lists
    table.T = T; table.M = M; table.R = (uint32_t)novel.size();
    table.offsets.clear();
    table.ids.clear();
    table.offsets.reserve(table.n_ecs() + 1);
    table.offsets.push_back(0);
    for (uint32_t t = 0; t < T; ++t) {
        table.ids.push_back(t);
        table.offsets.push_back(table.ids.size());
    }
    for (uint32_t c = 0; c < num_classes; ++c) {
        if (class_ec[c] == CLASS_EC_NONE || ec_offset[c + 1] - ec_offset[c] < 2) continue;
        table.ids.insert(table.ids.end(), ec_ids + ec_offset[c], ec_ids + ec_offset[c + 1]);
        table.offsets.push_back(table.ids.size());
    }
    for (const uint64_t l : novel) {
        table.ids.insert(table.ids.end(), list_ids + list_off[l], list_ids + list_off[l + 1]);
        table.offsets.push_back(table.ids.size());
    }
    return PA_OK;
}

std::string bus_header(uint32_t bc_len, uint32_t umi_len) {
    std::string s("BUS\0", 4);
    put_le32(s, 1);
    put_le32(s, bc_len);
    put_le32(s, umi_len);
    put_le32(s, 0);   // no free text
    return s;
}

std::string matrix_ec_text(const EcTable& table) {
    std::string out;
    const uint64_t n = table.n_ecs();
    out.resize((size_t)(n * 12 + table.ids.size() * 11 + 1));   // "ec\t" and "\n" per line, "id," per id: never more
    char* p = &out[0];
    for (uint64_t e = 0; e < n; ++e) {
        p = put_u64(p, e);
        *p++ = '\t';
        for (uint64_t j = table.offsets[e]; j < table.offsets[e + 1]; ++j) {
            if (j > table.offsets[e]) *p++ = ',';
            p = put_u64(p, table.ids[j]);
        }
        *p++ = '\n';
    }
    out.resize((size_t)(p - out.data()));
    return out;
}

std::string transcripts_text(const std::vector<std::string>& names) {
    std::string out;
    for (const std::string& n : names) {
        out += n;
        out += '\n';
    }
    return out;
}

int write_files(const char* out_dir, uint32_t bc_len, uint32_t umi_len, const RecordSource& next, const EcTable& table, const std::vector<std::string>& names) {
    struct stat sd;
    if (stat(out_dir, &sd) != 0 || !S_ISDIR(sd.st_mode)) return fail(PA_ERR_IO, "%s is no directory", out_dir);
    static_assert(sizeof(pa_bus_record) == 32, "pa_bus_record is the file's record");
    const std::string dir(out_dir), path = dir + "/output.bus";
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return fail(PA_ERR_IO, "cannot create %s: %s", path.c_str(), strerror(errno));
    const std::string head = bus_header(bc_len, umi_len);
    bool ok = fwrite(head.data(), 1, head.size(), f) == head.size();
    int e = PA_OK;
    while (ok) {
        const pa_bus_record* records = nullptr;
        uint64_t n = 0;
        if ((e = next(&records, &n)) != PA_OK || n == 0) break;
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__
        ok = fwrite(records, 32, (size_t)n, f) == n;   // the struct in memory is the record of the file
#else
        std::string body;   // a big-endian host writes the fields byte by byte
        body.reserve((size_t)n * 32);
        for (uint64_t i = 0; i < n; ++i) {
            const pa_bus_record& r = records[i];
            put_le64(body, r.barcode);
            put_le64(body, r.umi);
            put_le32(body, (uint32_t)r.ec);
            put_le32(body, r.count);
            put_le32(body, r.flags);
            put_le32(body, r.pad);
        }
        ok = fwrite(body.data(), 1, body.size(), f) == body.size();
#endif
    }
    if (fclose(f) != 0) ok = false;
    if (e != PA_OK) return e;
    if (!ok) return fail(PA_ERR_IO, "cannot write %s", path.c_str());
    if ((e = write_all(dir + "/matrix.ec", matrix_ec_text(table))) != PA_OK) return e;
    return write_all(dir + "/transcripts.txt", transcripts_text(names));
}

int write_files(const char* out_dir, uint32_t bc_len, uint32_t umi_len, const pa_bus_record* records, uint64_t n_records, const EcTable& table,
                const std::vector<std::string>& names) {
    bool given = false;
    return write_files(out_dir, bc_len, umi_len, [&](const pa_bus_record** p, uint64_t* n) {
        *p = records;
        *n = given ? 0 : n_records;
        given = true;
        return (int)PA_OK;
    }, table, names);
}

}  // namespace bus
}  // namespace pa
