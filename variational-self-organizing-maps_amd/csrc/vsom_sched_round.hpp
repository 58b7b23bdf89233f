// vsom_sched_round.hpp -- the "round image" of a resident schedule: what one round of at most
// VSOM_SCHEDULE_MAX_EPOCHS epochs of the one-launch schedule kernels reads besides the members' own state, as ONE host
// image that the caller copies to the device once:
//   tables     one neighbourhood table of lw x lh floats per distinct (lw, lh, sigma's bits), in the order of first use
//   offsets    for every member in member order, one unsigned per epoch of the round: its table's first float
//   validity   the members' validity bytes as given, packed in member order (a plain member has none)
// Host C++ only, no HIP: the single-context schedules (vsom_tiny.hip) and the ensemble's (vsom_ensemble.hip) build their
// rounds here, and tests/sched_round_driver.cpp pins the layout without a device.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

extern "C" double vsom_neighbourhood_weight(size_t cx, size_t cy, size_t bx, size_t by, double sigma);

// the tables of a round: one per distinct (lut_w, lut_h, sigma), packed in the order of first use
struct VsomSchedTables {
    std::map<std::tuple<uint32_t, uint32_t, uint64_t>, size_t> at;   // (shape, sigma's bits) -> the table's first float
    size_t floats = 0;
    size_t add(uint32_t w, uint32_t h, double sigma)                 // the table's first float
    {
        uint64_t bits;
        std::memcpy(&bits, &sigma, sizeof(bits));
        const auto r = at.emplace(std::make_tuple(w, h, bits), floats);
        if (r.second)
            floats += (size_t)w * h;
        return r.first->second;
    }
    void tabulate(float *host) const                                 // every table, as ensure_lut fills one
    {
        for (const auto &kv : at) {
            const uint32_t w = std::get<0>(kv.first), h = std::get<1>(kv.first);
            double sigma;
            std::memcpy(&sigma, &std::get<2>(kv.first), sizeof(sigma));
            float *t = host + kv.second;
            for (uint32_t dy = 0; dy < h; ++dy)
                for (uint32_t dx = 0; dx < w; ++dx)
                    t[(size_t)dy * w + dx] = (float)vsom_neighbourhood_weight(dx, dy, 0, 0, sigma);
        }
    }
};

// one participating member's share of a round
struct VsomSchedMember {
    uint32_t lw, lh;             // its table's shape (vsom_lut_dims)
    const double *sigma;         // the round's slice of its sigmas
    size_t epochs;               // ... 0 to VSOM_SCHEDULE_MAX_EPOCHS of them (0: its schedule has ended)
    const uint8_t *valid;        // its validity bytes, or null
    size_t vbytes;               // ... and their count (0: a plain member, or one whose bytes travel another way)
};

struct VsomSchedRound {
    VsomSchedTables tabs;
    std::vector<unsigned> tab;           // the offsets region
    std::vector<size_t> tab_at, v_at;    // per member: its first offset word; its validity bytes within their region
    size_t vtotal = 0;

    size_t table_bytes() const { return tabs.floats * sizeof(float); }
    size_t offset_bytes() const { return tab.size() * sizeof(unsigned); }
    size_t valid_bytes() const { return vtotal; }
    size_t bytes() const { return table_bytes() + offset_bytes() + valid_bytes(); }

    // lays the round out; false: its tables exceed 2^32 values (an offset word could not name them).  A member with no
    // epochs left contributes neither offsets nor validity bytes.
    bool plan(const VsomSchedMember *m, size_t n)
    {
        tabs = VsomSchedTables();
        tab.clear();
        tab_at.assign(n, 0);
        v_at.assign(n, 0);
        vtotal = 0;
        for (size_t k = 0; k < n; ++k) {
            if (!m[k].epochs)
                continue;
            tab_at[k] = tab.size();
            for (size_t ep = 0; ep < m[k].epochs; ++ep)
                tab.push_back((unsigned)tabs.add(m[k].lw, m[k].lh, m[k].sigma[ep]));
            v_at[k] = vtotal;
            vtotal += m[k].vbytes;
        }
        return tabs.floats <= 0xFFFFFFFFull;
    }

    // the image of the planned round into `host` (bytes() of it)
    void write(unsigned char *host, const VsomSchedMember *m) const
    {
        tabs.tabulate(reinterpret_cast<float *>(host));
        if (!tab.empty())
            std::memcpy(host + table_bytes(), tab.data(), offset_bytes());
        unsigned char *v = host + table_bytes() + offset_bytes();
        for (size_t k = 0; k < tab_at.size(); ++k)
            if (m[k].epochs && m[k].vbytes)
                std::memcpy(v + v_at[k], m[k].valid, m[k].vbytes);
    }
};
