// plan_window (csrc/fastq_text.cpp) over made-up texts: no file, no GPU. A stand-alone host program (tests/plan/build.py builds it under AddressSanitizer +
// UndefinedBehaviorSanitizer, tests/test_plan_window.py runs it). Every text is walked plan by plan, as pa_process_reads walks it, and the plans are held
// against the function's contract; then the walk is restarted inside members, as behind a discarded window. Prints one line per case, exits 1 on a miss.
#include <cstdio>
#include <string>
#include <vector>

#include "fastq_text.hpp"

namespace pa {   // (what fastq_text.cpp needs of the library's error plumbing)
std::string& last_error_ref() { static std::string s; return s; }
int fail(int code, const char*, ...) { return code; }
}  // namespace pa

using namespace pa::ingest;

static int misses = 0;
#define EXPECT(cond, ...)                                                       \
    do {                                                                        \
        if (!(cond)) { ++misses; printf("MISS %s:%d %s: ", name, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

static FastqText plain_text(uint64_t size) {
    FastqText t;
    t.fsize = size;
    return t;
}

// a BGZF text of members with these ISIZEs: 18 bytes of header, a payload of a third of the text + 2, 8 bytes of trailer each
static FastqText bgzf_text(const std::vector<uint32_t>& out_lens) {
    FastqText t;
    t.bgzf = true;
    uint64_t file = 0, out = 0;
    for (const uint32_t n : out_lens) {
        pa_bgzf_member m = {};
        m.file_off = file;
        m.in_off = file + 18;
        m.in_len = n / 3 + 2;
        m.out_off = out;
        m.out_len = n;
        t.members.push_back(m);
        file += 18 + m.in_len + 8;
        out += n;
    }
    t.map_size = file;
    t.fsize = out;
    return t;
}

static uint64_t end_of(const FastqText& t, uint64_t m) { return t.members[m].out_off + t.members[m].out_len; }

static void walk(const char* name, const FastqText& t, uint64_t W, uint64_t KEEP) {
    const uint64_t host_from = t.fsize > KEEP ? t.fsize - KEEP : 0;   // no plan reaches past it
    uint64_t read_to = 0, plans = 0;
    for (;; ++plans) {
        const WindowPlan p = plan_window(t, read_to, W, KEEP);
        if (!p.active) break;
        EXPECT(p.text_from == read_to, "plan %llu starts at %llu, the one before ended at %llu", (unsigned long long)plans, (unsigned long long)p.text_from, (unsigned long long)read_to);
        EXPECT(p.text_len >= 1 && p.text_len <= W, "plan %llu has %llu bytes of text", (unsigned long long)plans, (unsigned long long)p.text_len);
        EXPECT(p.text_from + p.text_len <= host_from, "plan %llu ends at %llu", (unsigned long long)plans, (unsigned long long)(p.text_from + p.text_len));
        if (t.bgzf) {
            const uint64_t m0 = p.first_member, m1 = m0 + p.n_members;
            EXPECT(p.n_members >= 1 && m1 <= t.members.size(), "plan %llu has %llu members", (unsigned long long)plans, (unsigned long long)p.n_members);
            if (p.n_members < 1 || m1 > t.members.size()) break;
            EXPECT(t.members[m0].out_off == p.text_from && t.members[m0].out_len > 0, "plan %llu does not start with a member's text", (unsigned long long)plans);
            EXPECT(end_of(t, m1 - 1) == p.text_from + p.text_len, "plan %llu does not end with a member's text", (unsigned long long)plans);
            EXPECT(p.comp_from == t.members[m0].file_off, "plan %llu: comp_from", (unsigned long long)plans);
            EXPECT(p.comp_len == (m1 < t.members.size() ? t.members[m1].file_off : t.map_size) - t.members[m0].file_off, "plan %llu: comp_len %llu", (unsigned long long)plans, (unsigned long long)p.comp_len);
            // behind a discarded window the walk restarts inside a member: the plan starts with that member's first byte
            for (uint64_t m = m0; m < m1; ++m) {
                if (t.members[m].out_len < 2) continue;
                for (const uint64_t inside : {t.members[m].out_off + 1, t.members[m].out_off + t.members[m].out_len / 2, end_of(t, m) - 1}) {
                    const WindowPlan q = plan_window(t, inside, W, KEEP);
                    EXPECT(q.active && q.first_member == m && q.text_from == t.members[m].out_off && q.text_from + q.text_len > inside,
                           "restart at %llu inside member %llu: active %d, from %llu", (unsigned long long)inside, (unsigned long long)m, (int)q.active, (unsigned long long)q.text_from);
                }
            }
        } else {
            EXPECT(p.n_members == 0 && p.comp_len == 0, "plan %llu of plain text names members", (unsigned long long)plans);
        }
        if (p.text_len == 0 || plans > t.fsize) { EXPECT(false, "the walk stalls at %llu", (unsigned long long)read_to); break; }
        read_to = p.text_from + p.text_len;
    }
    // the walk has ended: what is left is the host's. Plain text: exactly the last KEEP bytes (all of a text no longer than that). BGZF: no whole member
    // fits any more between read_to and the host's part, or within W
    if (!t.bgzf) EXPECT(read_to == host_from, "the walk ended at %llu of %llu", (unsigned long long)read_to, (unsigned long long)t.fsize);
    else if (read_to < host_from) {
        const uint64_t m = bgzf_member_at(t, read_to);
        EXPECT(t.members[m].out_off == read_to && (end_of(t, m) > host_from || t.members[m].out_len > W), "the walk ended at %llu in front of a member that fits", (unsigned long long)read_to);
    }
    EXPECT(!plan_window(t, read_to, W, KEEP).active && !plan_window(t, t.fsize, W, KEEP).active, "a plan behind the end");
    printf("%s: %llu bytes, %llu plans, the host's part from %llu\n", name, (unsigned long long)t.fsize, (unsigned long long)plans, (unsigned long long)read_to);
}

int main() {
    const uint64_t W = 1 << 20, KEEP = 1 << 18;
    walk("plain, empty", plain_text(0), W, KEEP);
    walk("plain, KEEP", plain_text(KEEP), W, KEEP);
    walk("plain, KEEP + 1", plain_text(KEEP + 1), W, KEEP);
    walk("plain, 3 W + 17", plain_text(3 * W + 17), W, KEEP);
    walk("plain, small window", plain_text(100000), 700, 4096);
    walk("bgzf, uniform", bgzf_text(std::vector<uint32_t>(100, 65280)), W, KEEP);
    walk("bgzf, uniform, the smallest window", bgzf_text(std::vector<uint32_t>(100, 65280)), PA_BGZF_MAX_ISIZE, 16384);
    walk("bgzf, empty members in front and between", bgzf_text({0, 0, 65280, 0, 65280, 65280, 0, 0, 0, 70, 65536, 0, 1, 65280, 65280, 65280, 65280, 65280, 0}), 3 * 65536, 65536);
    walk("bgzf, a member larger than the window", bgzf_text({3000, 3000, 65536, 3000, 3000, 3000, 3000}), 10000, 4096);
    walk("bgzf, the last member ends at fsize - KEEP", bgzf_text({65280, 65280, 65280, 65280, 40000, 25536}), 2 * 65536, 65536);
    walk("bgzf, nothing but the host's part", bgzf_text({3000, 0}), W, 4096);
    printf("%s\n", misses ? "FAILED" : "OK");
    return misses ? 1 : 0;
}
