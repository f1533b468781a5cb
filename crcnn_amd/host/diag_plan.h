// diag_plan.h -- the plan of the diagonal matrix-vector product over slots (matvecSlots, crcnn_host.h), header only: no engine, no device.
// W (out x in, out and in <= M) is taken as zero-padded to M x M, M a power of two <= n/2.  For every diagonal d with a non-zero entry: steps gets d and rows gets
// n more words, rows[r][i] = W[i mod M][(i mod M + d) mod M] -- period M over both rows of n/2 slots.  false (nothing written) for a bad M or shape.
#pragma once
#include <cstdint>
#include <vector>

inline bool crc_diag_plan(const std::vector<std::vector<int64_t>> &W, int M, int n, std::vector<int> &steps, std::vector<int64_t> &rows)
{
    if (M < 1 || (M & (M - 1)) || n < 2 || M > n / 2 || (int)W.size() > M) return false;
    for (auto &r : W) if ((int)r.size() > M) return false;
    steps.clear(); rows.clear();
    std::vector<int64_t> diag((size_t)M);
    for (int d = 0; d < M; d++) {
        bool any = false;
        for (int i = 0; i < M; i++) {
            const int j = (i + d) % M;
            diag[i] = i < (int)W.size() && j < (int)W[i].size() ? W[i][j] : 0;
            any = any || diag[i] != 0;
        }
        if (!any) continue;
        steps.push_back(d);
        for (int i = 0; i < n; i++) rows.push_back(diag[i % M]);
    }
    return true;
}
