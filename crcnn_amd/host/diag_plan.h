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

// ---- baby-step / giant-step (matvecSlotsBsgs; crc_diag_mac_bsgs_forms) ----
// A diagonal d = B j + b (0 <= b < B, B a power of two, 1 <= B <= M) is reached as rotate(., B j) of a product with rotate(x, b):
//     y = Sum_j rotate_rows( Sum_b rows[j][b] (.) rotate_rows(x, b), B j ),   rows[j][b][i] = W[(i - B j) mod M][(i + b) mod M]
// (the diagonal d, rotated back by the giant step that follows the product; period M over both rows of n/2 slots).  giant_steps gets B j for every group j
// with a non-zero entry, baby_steps every b with a non-zero entry in a kept group, rows [giant][baby][n] with zero rows where a pair (j, b) is empty.
// Preconditions as crc_diag_plan, plus those on B; false (nothing written) otherwise.
inline bool crc_bsgs_plan(const std::vector<std::vector<int64_t>> &W, int M, int n, int B, std::vector<int> &baby_steps, std::vector<int> &giant_steps,
                          std::vector<int64_t> &rows)
{
    if (M < 1 || (M & (M - 1)) || n < 2 || M > n / 2 || (int)W.size() > M || B < 1 || (B & (B - 1)) || B > M) return false;
    for (auto &r : W) if ((int)r.size() > M) return false;
    auto at = [&](int i, int j) -> int64_t { return i < (int)W.size() && j < (int)W[i].size() ? W[i][j] : 0; };
    std::vector<char> used((size_t)M, 0), baby((size_t)B, 0);           // diagonals with a non-zero entry; baby steps with one
    for (int d = 0; d < M; d++)
        for (int i = 0; i < M && !used[d]; i++) used[d] = at(i, (i + d) % M) != 0;
    baby_steps.clear(); giant_steps.clear(); rows.clear();
    for (int j = 0; j < M / B; j++) {
        bool any = false;
        for (int b = 0; b < B; b++) if (used[B * j + b]) { any = true; baby[b] = 1; }
        if (any) giant_steps.push_back(B * j);
    }
    for (int b = 0; b < B; b++) if (baby[b]) baby_steps.push_back(b);
    for (int gs : giant_steps)
        for (int b : baby_steps)
            for (int i = 0; i < n; i++) rows.push_back(at(((i - gs) % M + M) % M, (i + b) % M));
    return true;
}
// the Galois elements of a dense M x M product split at B: 3^s mod 2n (crc_galois_elt_rows) of every baby step 1 .. B - 1 and every giant step B, 2 B, .. M - B,
// each once, in that order -- the key set to generate.  Empty for bad arguments (those of crc_bsgs_plan) and for M = 1
inline std::vector<uint64_t> crc_bsgs_elements(int M, int B, int n)
{
    std::vector<uint64_t> out;
    if (M < 1 || (M & (M - 1)) || n < 2 || M > n / 2 || B < 1 || (B & (B - 1)) || B > M) return out;
    const uint64_t mask = 2 * (uint64_t)n - 1;
    uint64_t g = 1;
    for (int s = 1; s < M; s++) {
        g = g * 3 & mask;
        if (s < B || s % B == 0) out.push_back(g);
    }
    return out;
}
