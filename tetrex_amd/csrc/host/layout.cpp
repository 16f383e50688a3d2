// The size-aware HIBF layout (see layout.hpp for the rules it follows).
#include "layout.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <numeric>
#include <stdexcept>
#include <string>

namespace tetrex {

uint64_t compute_bitcount(uint64_t n, float fpr) {
    const double num = -static_cast<double>(n) * std::log(fpr);  // float log, as in the reference
    const double den = std::pow(std::log(2), 2);
    return static_cast<uint64_t>(std::ceil(num / den));
}

uint64_t default_tmax(uint64_t user_bins) { return 64 * (((uint64_t)std::ceil(std::sqrt((double)user_bins)) + 63) / 64); }

uint64_t union_window(uint64_t user_bins, uint64_t tmax) { return std::min(user_bins, 4 * ((user_bins + tmax - 1) / tmax)); }

std::vector<uint64_t> layout_order(const double* counts, uint64_t user_bins) {
    std::vector<uint64_t> order(user_bins);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return counts[a] > counts[b]; });
    return order;
}

std::vector<double> split_corrections(uint64_t max_parts, double fpr, unsigned hash_count) {
    std::vector<double> corr(max_parts + 1, 1.0);
    const double num = std::log(1.0 - std::pow(fpr, 1.0 / hash_count));
    for (uint64_t s = 2; s <= max_parts; ++s) {
        const double p = 1.0 - std::pow(1.0 - fpr, 1.0 / (double)s);
        corr[s] = num / std::log(1.0 - std::pow(p, 1.0 / hash_count));
    }
    return corr;
}

namespace {

struct Cell {
    double score = std::numeric_limits<double>::infinity();
    double maxw = 0, low = 0;
    uint32_t len = 0;  // split: parts (technical bins); merge: bins in the run
    bool merge = false;
    bool ok() const { return std::isfinite(score); }
};

struct Ctx {
    const double* counts;  // by user bin
    const double* unions;  // sorted position x window
    uint64_t window, tmax;
    const std::vector<uint64_t>* order;
    std::vector<double> corr;
    LayoutParams p;
    HibfLayout* out;

    double c(uint64_t pos) const { return counts[(*order)[pos]]; }
    double u(uint64_t start, uint64_t len) const { return unions[start * window + len - 1]; }

    // lays out sorted positions [lo, hi) as one IBF and its sub-trees; returns its id
    uint64_t layout(uint64_t lo, uint64_t hi) {
        const uint64_t n = hi - lo, T = std::min(tmax, 64 * ((n + 63) / 64));
        const uint64_t id = out->ibfs.size();
        out->ibfs.emplace_back();
        std::vector<Cell> M(T * n);
        auto at = [&](uint64_t i, uint64_t j) -> Cell& { return M[i * n + j]; };
        // depth of a run of L bins below a merged bin: ceil(log_T(L))
        auto depth = [&](uint64_t L) {
            double d = 0;
            for (uint64_t cap = 1; cap < L; cap *= T) d += 1;
            return d;
        };
        std::vector<double> prefix(n + 1, 0.0);
        for (uint64_t j = 0; j < n; ++j) prefix[j + 1] = prefix[j] + c(lo + j);
        for (uint64_t j = 0; j < n; ++j) {
            for (uint64_t i = 0; i < T; ++i) {
                Cell& best = at(i, j);
                auto offer = [&](double maxw, double low, uint32_t len, bool merge) {
                    const double score = (double)(i + 1) * maxw + p.alpha * low;
                    if (score < best.score) best = Cell{score, maxw, low, len, merge};
                };
                // split (s = 1: the bin alone in one technical bin)
                for (uint64_t s = 1; s <= i + 1; ++s) {
                    const double w = std::ceil(c(lo + j) / (double)s) * corr[s];
                    if (j == 0) {
                        if (s == i + 1) offer(w, 0.0, (uint32_t)s, false);
                    } else if (s <= i) {
                        const Cell& prev = at(i - s, j - 1);
                        if (prev.ok()) offer(std::max(prev.maxw, w), prev.low, (uint32_t)s, false);
                    }
                }
                // merge of bins j-L+1 .. j
                for (uint64_t L = 2; L <= std::min<uint64_t>(window, j + 1); ++L) {
                    const uint64_t first = j + 1 - L;
                    const double w = u(lo + first, L), low = (prefix[j + 1] - prefix[first]) * depth(L);
                    if (first == 0) {
                        if (i == 0) offer(w, low, (uint32_t)L, true);
                    } else if (i >= 1) {
                        const Cell& prev = at(i - 1, first - 1);
                        if (prev.ok()) offer(std::max(prev.maxw, w), prev.low + low, (uint32_t)L, true);
                    }
                }
            }
        }
        if (!at(T - 1, n - 1).ok())
            throw std::invalid_argument("no layout of " + std::to_string(n) + " user bins in " + std::to_string(T) +
                                        " technical bins with runs of at most " + std::to_string(window));
        // walk back: technical bins from the last to the first
        struct Tb { bool merge; uint64_t first, len; };  // merge: sorted run [first, first+len); split: bin `first`, len parts
        std::vector<Tb> tbs;
        for (int64_t i = (int64_t)T - 1, j = (int64_t)n - 1; j >= 0;) {
            const Cell& cell = at((uint64_t)i, (uint64_t)j);
            if (cell.merge) {
                tbs.push_back({true, (uint64_t)(j + 1 - cell.len), cell.len});
                j -= cell.len;
                i -= 1;
            } else {
                for (uint32_t s = 0; s < cell.len; ++s) tbs.push_back({false, (uint64_t)j, cell.len});
                j -= 1;
                i -= cell.len;
            }
        }
        std::reverse(tbs.begin(), tbs.end());
        uint64_t rows = 1;
        std::vector<uint64_t> next(T, 0), user(T, 0);
        for (uint64_t t = 0; t < T; ++t) {
            const Tb& b = tbs[t];
            if (b.merge) {
                user[t] = UINT64_MAX;
                rows = std::max(rows, compute_bitcount((uint64_t)std::ceil(u(lo + b.first, b.len)), p.relaxed_fpr));
            } else {
                user[t] = (*order)[lo + b.first];
                const double part = std::ceil(c(lo + b.first) / (double)b.len);
                rows = std::max(rows, compute_bitcount((uint64_t)std::ceil(part * corr[b.len]), p.fpr));
            }
        }
        for (uint64_t t = 0; t < T; ++t)
            if (tbs[t].merge) next[t] = layout(lo + tbs[t].first, lo + tbs[t].first + tbs[t].len);
        LayoutIbf& me = out->ibfs[id];
        me.bin_size = rows;
        me.next_ibf_id = std::move(next);
        me.tb_to_user_bin = std::move(user);
        return id;
    }
};

}  // namespace

std::vector<uint64_t> rearrange_intervals(const double* counts, const uint64_t* order, uint64_t user_bins, double ratio, uint64_t max_len) {
    if (!(ratio > 0 && ratio <= 1)) throw std::invalid_argument("the rearrangement ratio must lie in (0, 1]");
    if (max_len < 1 || max_len > kRearrangeMaxLen)
        throw std::invalid_argument("an interval holds 1 .. " + std::to_string(kRearrangeMaxLen) + " bins at most");
    if (user_bins && (!counts || !order)) throw std::invalid_argument("null argument");
    std::vector<uint64_t> starts;
    for (uint64_t s = 0; s < user_bins;) {
        starts.push_back(s);
        const double floor = ratio * counts[order[s]];
        uint64_t e = s + 1;
        while (e < user_bins && e - s < max_len && counts[order[e]] >= floor) ++e;
        s = e;
    }
    return starts;
}

std::vector<uint64_t> rearrange_chain(const double* counts, const double* unions, uint64_t n) {
    if (n && (!counts || !unions)) throw std::invalid_argument("null argument");
    std::vector<uint64_t> chain(n);
    std::iota(chain.begin(), chain.end(), 0);
    if (n < 3) return chain;
    std::vector<uint8_t> placed(n, 0);
    placed[0] = 1;
    for (uint64_t k = 1; k < n; ++k) {
        const uint64_t last = chain[k - 1];
        uint64_t best = n;
        double best_j = 0;
        for (uint64_t j = 0; j < n; ++j) {
            if (placed[j]) continue;
            const double u = unions[last * n + j];
            const double jac = u == 0 ? 0.0 : (counts[last] + counts[j] - u) / u;
            if (best == n || jac > best_j) { best = j; best_j = jac; }  // ascending j: the smaller position keeps a tie
        }
        chain[k] = best;
        placed[best] = 1;
    }
    return chain;
}

HibfLayout hibf_layout(const double* counts, uint64_t user_bins, const double* unions, uint64_t window, const LayoutParams& params) {
    if (user_bins == 0 || !counts || !unions) throw std::invalid_argument("no user bins");
    for (uint64_t b = 0; b < user_bins; ++b)  // before they are sorted
        if (!(counts[b] >= 0) || !std::isfinite(counts[b])) throw std::invalid_argument("counts must be finite and >= 0");
    const std::vector<uint64_t> order = layout_order(counts, user_bins);
    return hibf_layout_ordered(counts, user_bins, order.data(), unions, window, params);
}

HibfLayout hibf_layout_ordered(const double* counts, uint64_t user_bins, const uint64_t* order, const double* unions, uint64_t window,
                               const LayoutParams& params) {
    if (user_bins == 0 || !counts || !unions || !order) throw std::invalid_argument("no user bins");
    const uint64_t tmax = params.tmax ? params.tmax : default_tmax(user_bins);
    if (tmax % 64) throw std::invalid_argument("t_max must be a multiple of 64");
    if (window != union_window(user_bins, tmax))
        throw std::invalid_argument("the union table's window must be min(B, 4 * ceil(B / t_max)) = " +
                                    std::to_string(union_window(user_bins, tmax)));
    if (!(params.fpr > 0 && params.fpr < 1) || !(params.relaxed_fpr > 0 && params.relaxed_fpr < 1) || params.hash_count < 1 ||
        params.hash_count > 5 || !(params.alpha >= 0))
        throw std::invalid_argument("fpr and relaxed_fpr must lie in (0, 1), hash_count in 1..5, alpha >= 0");
    for (uint64_t b = 0; b < user_bins; ++b)
        if (!(counts[b] >= 0) || !std::isfinite(counts[b])) throw std::invalid_argument("counts must be finite and >= 0");
    {
        std::vector<uint8_t> seen(user_bins, 0);
        for (uint64_t s = 0; s < user_bins; ++s) {
            if (order[s] >= user_bins || seen[order[s]])
                throw std::invalid_argument("the order must be a permutation of the user bins 0 .. " + std::to_string(user_bins - 1));
            seen[order[s]] = 1;
        }
    }
    HibfLayout out;
    out.tmax = tmax;
    out.window = window;
    out.order.assign(order, order + user_bins);
    Ctx ctx{counts, unions, window, tmax, &out.order, split_corrections(tmax, params.fpr, params.hash_count), params, &out};
    ctx.p.tmax = tmax;
    ctx.layout(0, user_bins);
    return out;
}

std::vector<std::vector<PathStep>> layout_paths(const HibfLayout& layout, uint64_t user_bins) {
    std::vector<std::vector<PathStep>> paths(user_bins);
    std::vector<PathStep> stack;
    auto walk = [&](auto&& self, uint64_t ibf) -> void {
        const LayoutIbf& f = layout.ibfs[ibf];
        const uint64_t T = f.tb_to_user_bin.size();
        for (uint64_t t = 0; t < T;) {
            if (f.tb_to_user_bin[t] == UINT64_MAX) {
                stack.push_back({ibf, t, 1});
                self(self, f.next_ibf_id[t]);
                stack.pop_back();
                ++t;
                continue;
            }
            const uint64_t ub = f.tb_to_user_bin[t];
            uint64_t e = t + 1;
            while (e < T && f.tb_to_user_bin[e] == ub) ++e;
            if (ub >= user_bins || !paths[ub].empty()) throw std::invalid_argument("user bin placed twice or out of range");
            paths[ub] = stack;
            paths[ub].push_back({ibf, t, e - t});
            t = e;
        }
    };
    walk(walk, 0);
    return paths;
}

}  // namespace tetrex
