// window_unpack_feature.hip -- the cell pairs window_unpack.hip counts, read as FEATURE SUMS: window_score_feature.hip's reading at cell
// level.
//
// The reference's LUAD notebook never reads metacell pairs (examples/luad/reproduce_figures.ipynb): cell 12 unpacks the metacell matches
// to cells, cell 16 gathers the PCF row and the Xenium row of every CELL pair, cell 18 takes the marker means per annotation of the
// moving cell, cell 20 the distance of every pair's reference cell to the nearest pair of a zone, cells 21-22 the marker means per bin of
// that distance over a subset of the pairs.  A metacell has no feature row and its annotation is not a cell's.  When a set's merge ends
// the unpack phases keep the cell pairs on the device (win::unpack_run with a win::PairReader) and the reference members' XY is
// resident (same_members); one feature row per MEMBER, the moving cells' groups and the per-member flags are constant over a study and
// uploaded once (same_unpack_features, same_unpack_zone).  same_merge_acc_unpack_features joins the two:
//
//   the reader's enqueue, behind the last solve launch:   feature_sums_kernel<PairSource> by the moving member's group; with a zone
//   win::feat::zone_phases<PairSource> -- the flag kernel, a 32-byte copy and a WAIT INSIDE THE READER (the host must know the zone
//   pairs' count and box before grid.h's build; PairReader is not given a second stage for it), the grid build, the walk, the sums by
//   distance bin --; then the copies of the sums, of d2 and of the pairs' reference members, which unpack_run's last wait covers.
//
// The kernels are feature_kernels.h's, instantiated over a pair of win::DevicePairs whose -1 means skip: nothing of them is stated here.
// A pair's rows are flat MEMBER indices, its bin is member_group[moving member], its position the reference member's XY, its d2 slot the
// pair itself -- so the call is well defined where hostile final rows name a moving row twice.
//
// The sums live in `unpack_feature` of the accumulator under the protocol of work_sets.h (the first kernel clears what the call before
// counted into the other set), the zone's scan words and totals in `unpack_zone` likewise; that one is laid where the pairs' number is
// known, inside the reader's enqueue and so inside the in-doubt window of the unpack buffer.
#include "feature_kernels.h"

#include <cstring>
#include <optional>

struct same_unpack_features {
    same_ctx *ctx = nullptr;
    const same_members *mov = nullptr, *ref = nullptr;
    int F_m = 0, F_r = 0, n_groups = 1;
    int32_t *mov_q = nullptr, *ref_q = nullptr;   // [mov->m][F_m], [ref->m][F_r]
    int32_t *member_group = nullptr;              // [mov->m] or null: every cell in group 0
};

struct same_unpack_zone {
    same_ctx *ctx = nullptr;
    const same_unpack_features *feats = nullptr;
    uint8_t *mov_flags = nullptr, *ref_flags = nullptr;   // per member; null: every bit set
    double *edges = nullptr;                              // [B + 1]
    int B = 0;
};

namespace {

using namespace win;
using namespace win::feat;

// the feature kernels as win::unpack_run's reader
struct FeatureReader : PairReader {
    same_merge_acc *a = nullptr;
    const same_members *mov = nullptr, *ref = nullptr;
    const same_unpack_features *feats = nullptr;
    const same_unpack_zone *zone = nullptr;
    FeatureLayout lo;
    bool ask_d2 = false, ask_ref = false;
    int64_t capacity = 0;
    // what comes back (the caller's arrays are written only by a call that succeeds)
    std::vector<unsigned long long> h;
    unsigned long long zt[ZONE_TOTALS] = {};
    std::vector<double> d2;
    std::vector<int64_t> ref_member;
    bool too_small = false, d2_copied = false;
    std::optional<InDoubt> zone_doubt;            // the zone work buffer: in doubt from the flag kernel to the call's last wait

    int lay(same_ctx *ctx) override {
        const int64_t words = lo.words();
        if (sets->fits(words)) return SAME_OK;
        InDoubt laying(*sets);
        SAME_TRY(lay_over(ctx, a->unpack_feature, a->ufw, words));
        SAME_FILL(ctx, a->unpack_feature.p, 0, a->ufw.bytes);
        sets->laid_anew(words);
        return SAME_OK;
    }
    int enqueue(same_ctx *ctx, const DevicePairs &p) override {
        const int64_t words = lo.words(), pairs = p.pairs;
        too_small = (ask_d2 || ask_ref) && capacity < pairs;
        const bool want_d2 = ask_d2 && !too_small, want_ref = ask_ref && !too_small;
        const PairSource src{p.ref_member, p.mov_member, pairs, mov->m, ref->m};
        ZoneWork zw;
        if (zone) {
            WorkSets &zs = a->unpack_zone_sets;
            if (!zs.fits(pairs)) {
                InDoubt laying(zs);
                SAME_TRY(lay_over(ctx, a->unpack_zone, zw, pairs));
                SAME_FILL(ctx, a->unpack_zone.p, 0, zw.zero_bytes);
                zs.laid_anew(pairs);
            }
            Carver place(a->unpack_zone.p);
            win::feat::lay(zw, place, zs.laid);
            zone_doubt.emplace(zs);
        }
        unsigned long long *bins = a->ufw.bins + (size_t)sets->set * a->ufw.cap, *next = a->ufw.bins + (size_t)(sets->set ^ 1) * a->ufw.cap;
        SAME_LAUNCH(ctx, feature_sums_kernel<PairSource>, sums_grid(pairs, lo.F, lo.G + 1), dim3(NT), 0, src, feats->member_group, 0, lo.G + 1,
                    lo.G, feats->mov_q, feats->F_m, feats->ref_q, feats->F_r, bins + lo.rows(), bins + lo.sums(), bins + lo.bad(), next,
                    sets->dirty);
        if (zone)
            SAME_TRY(zone_phases(ctx, "same_merge_acc_unpack_features: a pair outside the members",
                                 "same_merge_acc_unpack_features: a zone or subset pair's reference member XY is not finite", src, zw,
                                 a->unpack_zone_sets.set, zone->mov_flags, zone->ref_flags, zone->edges, lo.B, ref->xy, want_d2, feats->mov_q,
                                 feats->F_m, feats->ref_q, feats->F_r, bins + lo.bin_rows(), bins + lo.bin_sums(), zt));
        HIP_TRY(ctx, hipGetLastError());
        SAME_COPY(ctx, h.data(), bins, (size_t)words * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        if (zone && want_d2) {
            d2.resize((size_t)pairs);
            SAME_COPY(ctx, d2.data(), zw.d2, (size_t)pairs * sizeof(double), hipMemcpyDeviceToHost);
            d2_copied = true;
        }
        if (want_ref) {
            ref_member.resize((size_t)pairs);
            SAME_COPY(ctx, ref_member.data(), p.ref_member, (size_t)pairs * sizeof(int64_t), hipMemcpyDeviceToHost);
        }
        counted = words;
        return SAME_OK;
    }
};

}  // namespace

extern "C" {

int same_unpack_features_create(const same_members *mov, const same_members *ref, const int32_t *mov_q, int F_m, const int32_t *ref_q, int F_r,
                                const int32_t *member_group, int n_groups, same_unpack_features **out) {
    if (!mov || !out) return SAME_EINVAL;
    same_ctx *ctx = mov->ctx;
    *out = nullptr;
    REQUIRE(ctx, ref && ref->ctx->device == ctx->device);
    SAME_TRY(check_columns(ctx, "same_unpack_features_create", mov_q, mov->m, F_m, ref_q, ref->m, F_r, member_group, n_groups));
    SAME_TRY(same_use(ctx));
    same_unpack_features *f = new (std::nothrow) same_unpack_features();
    if (!f) return SAME_ENOMEM;
    f->ctx = ctx;
    f->mov = mov;
    f->ref = ref;
    f->F_m = F_m;
    f->F_r = F_r;
    f->n_groups = n_groups;
    *out = f;                                     // freed by the caller's destroy on any failure below
    SAME_TRY(upload(ctx, &f->mov_q, mov_q, (size_t)(mov->m * F_m)));
    SAME_TRY(upload(ctx, &f->ref_q, ref_q, (size_t)(ref->m * F_r)));
    SAME_TRY(upload(ctx, &f->member_group, member_group, (size_t)mov->m));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SAME_OK;
}

void same_unpack_features_destroy(same_unpack_features *f) {
    if (!f) return;
    (void)hipSetDevice(f->ctx->device);
    (void)hipDeviceSynchronize();                 // calls of other contexts may still be reading it
    if (f->mov_q) (void)hipFree(f->mov_q);
    if (f->ref_q) (void)hipFree(f->ref_q);
    if (f->member_group) (void)hipFree(f->member_group);
    delete f;
}

int same_unpack_zone_create(const same_unpack_features *feats, const uint8_t *mov_flags, const uint8_t *ref_flags, const double *d2_edges,
                            int n_edges, same_unpack_zone **out) {
    if (!feats || !out) return SAME_EINVAL;
    same_ctx *ctx = feats->ctx;
    *out = nullptr;
    SAME_TRY(check_edges(ctx, d2_edges, n_edges));
    SAME_TRY(same_use(ctx));
    same_unpack_zone *z = new (std::nothrow) same_unpack_zone();
    if (!z) return SAME_ENOMEM;
    z->ctx = ctx;
    z->feats = feats;
    z->B = n_edges - 1;
    *out = z;                                     // freed by the caller's destroy on any failure below
    SAME_TRY(upload(ctx, &z->mov_flags, mov_flags, (size_t)feats->mov->m));
    SAME_TRY(upload(ctx, &z->ref_flags, ref_flags, (size_t)feats->ref->m));
    SAME_TRY(upload(ctx, &z->edges, d2_edges, (size_t)n_edges));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SAME_OK;
}

void same_unpack_zone_destroy(same_unpack_zone *z) {
    if (!z) return;
    (void)hipSetDevice(z->ctx->device);
    (void)hipDeviceSynchronize();                 // calls of other contexts may still be reading it
    if (z->mov_flags) (void)hipFree(z->mov_flags);
    if (z->ref_flags) (void)hipFree(z->ref_flags);
    if (z->edges) (void)hipFree(z->edges);
    delete z;
}

int same_merge_acc_unpack_features(same_merge_acc *a, const same_members *mov, const same_members *ref, int strategy,
                                   const same_unpack_features *feats, const same_unpack_zone *zone, int64_t *out, int64_t out_words,
                                   double *out_d2, int64_t *out_ref_member, int64_t capacity) {
    if (!a) return SAME_EINVAL;
    same_ctx *ctx = a->ctx;
    REQUIRE(ctx, out && mov && ref);
    REQUIRE(ctx, feats && feats->mov == mov && feats->ref == ref && feats->ctx->device == ctx->device);
    REQUIRE(ctx, !zone || zone->feats == feats);
    REQUIRE(ctx, (!out_d2 && !out_ref_member) || capacity >= 0);
    FeatureReader reader;
    reader.a = a;
    reader.mov = mov;
    reader.ref = ref;
    reader.feats = feats;
    reader.zone = zone;
    reader.lo.G = feats->n_groups;
    reader.lo.F = feats->F_m + feats->F_r;
    reader.lo.B = zone ? zone->B : 0;
    reader.ask_d2 = out_d2 != nullptr;
    reader.ask_ref = out_ref_member != nullptr;
    reader.capacity = capacity;
    reader.sets = &a->unpack_feature_sets;
    const FeatureLayout &lo = reader.lo;
    REQUIRE(ctx, out_words >= 4 + lo.out_words());
    reader.h.assign((size_t)lo.words(), 0ull);
    int64_t counts[4] = {0, 0, 0, 0};
    SAME_TRY(unpack_run(a, mov, ref, strategy, counts, nullptr, 0, &reader));
    if (reader.zone_doubt) {                      // the last wait returned: the zone work buffer is sound, its other set the next call's
        reader.zone_doubt->sound();
        a->unpack_zone_sets.flip();
    }
    for (int q = 0; q < 4; ++q) out[q] = counts[q];
    if (reader.too_small) {
        ctx->err = "same_merge_acc_unpack_features: out_d2 / out_ref_member hold fewer than out[1] entries";
        return SAME_EINVAL;
    }
    const int64_t pairs = counts[1];
    int64_t *f = out + 4;
    for (int64_t q = 0; q < lo.out_words(); ++q) f[q] = (int64_t)reader.h[(size_t)q];
    f[0] = pairs;
    f[1] = pairs - f[lo.rows() + lo.G];
    f[2] = (int64_t)reader.zt[Z_ZONE];
    f[3] = (int64_t)reader.zt[Z_SUBSET];
    if (out_d2) {
        if (reader.d2_copied) std::memcpy(out_d2, reader.d2.data(), (size_t)pairs * sizeof(double));
        else
            for (int64_t i = 0; i < pairs; ++i) out_d2[i] = std::nan("");
    }
    if (out_ref_member && pairs > 0) std::memcpy(out_ref_member, reader.ref_member.data(), (size_t)pairs * sizeof(int64_t));
    return SAME_OK;
}

}  // extern "C"
