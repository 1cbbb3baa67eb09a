// host_check.h — what the stand-alone host checks (reach_host_check.cpp, read_best_host_check.cpp,
// consensus_host_check.cpp) share: the context helpers an API file links against, stubbed; EXPECT; a builder of
// sequence sets; and local_alignment on plain full tables.  The plain restatements here are the checks' oracle, so
// they are written out again and call nothing of csrc/ovl_local_host.h, the code under test.
#pragma once

#include <cstdarg>

#include "ovl_ctx.h"

thread_local std::string g_err;

int fail(const ovl_ctx*, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
int fail(const Dev*, int code, const char* fmt, ...) {
    g_err = fmt;
    return code;
}
void quiet(ovl_ctx*) {}

static int g_failed = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                     \
        }                                                                   \
    } while (0)

struct Seqs {
    std::vector<uint8_t> bytes;
    std::vector<int64_t> off{0};
    void add(const std::string& s) {
        bytes.insert(bytes.end(), s.begin(), s.end());
        off.push_back((int64_t)bytes.size());
    }
    int32_t n() const { return (int32_t)off.size() - 1; }
    std::string at(int32_t k) const { return std::string(bytes.begin() + off[k], bytes.begin() + off[k + 1]); }
    const uint8_t* data() const { return bytes.empty() ? nullptr : bytes.data(); }
    int64_t total() const { return (int64_t)bytes.size(); }
};

struct Triple {
    int64_t score, start, end;
};

// aligners.py:85-167 on full tables: the best score and the columns where the walk stops and starts; on_op(i, j, op)
// for every op of the walk (1 diag, 2 up, 3 left), taken at cell (i, j)
template <typename OnOp>
Triple local_plain(const std::string& q, const std::string& t, int64_t match, int64_t mismatch, int64_t indel,
                   OnOp&& on_op) {
    const size_t n = q.size(), m = t.size();
    std::vector<std::vector<int64_t>> dp(n + 1, std::vector<int64_t>(m + 1, 0));
    std::vector<std::vector<int>> tb(n + 1, std::vector<int>(m + 1, 0));
    int64_t best = 0;
    size_t bi = 0, bj = 0;
    for (size_t i = 1; i <= n; ++i)
        for (size_t j = 1; j <= m; ++j) {
            const int64_t d = dp[i - 1][j - 1] + (q[i - 1] == t[j - 1] ? match : mismatch);
            const int64_t u = dp[i - 1][j] + indel, l = dp[i][j - 1] + indel;
            if (d >= u && d >= l && d >= 0) { dp[i][j] = d; tb[i][j] = 1; }
            else if (u >= l && u >= 0) { dp[i][j] = u; tb[i][j] = 2; }
            else if (l >= 0) { dp[i][j] = l; tb[i][j] = 3; }
            if (dp[i][j] > best) { best = dp[i][j]; bi = i; bj = j; }
        }
    size_t i = bi, j = bj;
    while (i > 0 && j > 0 && dp[i][j] > 0) {
        const int op = tb[i][j];
        if (op < 1 || op > 3) break;
        on_op(i, j, op);
        if (op != 3) --i;
        if (op != 2) --j;
    }
    return {best, (int64_t)j, (int64_t)bj};
}
inline Triple local_plain(const std::string& q, const std::string& t, int64_t match, int64_t mismatch,
                          int64_t indel) {
    return local_plain(q, t, match, mismatch, indel, [](size_t, size_t, int) {});
}
