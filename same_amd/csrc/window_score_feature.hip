// window_score_feature.hip -- a merged result read as FEATURE SUMS: the matched pairs put two feature matrices side by side, and the sums
// of their rows per group of the moving rows and per bin of the distance to a marked zone are what the means of a study are made from.
//
// The reference's notebooks end every study this way (examples/luad/reproduce_figures.ipynb cells 16-22): the PCF rows and the Xenium rows
// of every matched pair gathered into one table, its mean per moving label (the matrixplot), cdist(X_spatial, zone).min(axis=1) per pair,
// pd.cut of that distance, the mean of a marker set per distance bin over a subset of the pairs.  When a set's merge ends the final rows
// and both sections' XY are resident; the feature matrices, the groups and the masks are constant over the study and uploaded once
// (same_score_features, same_feature_zone).  same_merge_acc_score_features reads them where they are:
//
//   feature_sums_kernel, zone_flag_kernel, (grid.h), zone_walk_kernel: feature_kernels.h states them once, over where a pair comes from --
//   here win::feat::FinalSource, a final row with followed(); same_merge_acc_unpack_features (window_unpack_feature.hip) reads cell pairs
//   through the same kernels.  The sums by group run first; with a zone, win::feat::zone_phases follows: flags and compaction, the wait for
//   the zone pairs' count, the grid build, the walk, the sums by distance bin.
//
// The sums live in the accumulator under the protocol of work_sets.h: two sets of the call's words, the first kernel clears what the call
// before counted into the other; the zone's scan words and totals likewise.  No other buffer of the accumulator is touched.
#include "feature_kernels.h"

struct same_score_features {
    same_ctx *ctx = nullptr;
    const same_section *mov = nullptr, *ref = nullptr;
    int F_m = 0, F_r = 0, n_groups = 1;
    int32_t *mov_q = nullptr, *ref_q = nullptr;   // [mov->n][F_m], [ref->n][F_r]
    int32_t *group_of = nullptr;                  // [mov->n] or null: every row in group 0
};

struct same_feature_zone {
    same_ctx *ctx = nullptr;
    const same_score_features *feats = nullptr;
    uint8_t *mov_flags = nullptr, *ref_flags = nullptr;   // null: every bit set
    double *edges = nullptr;                              // [B + 1]
    int B = 0;
};

using namespace win;
using namespace win::feat;

extern "C" {

int same_score_features_create(const same_section *mov, const same_section *ref, const int32_t *mov_q, int F_m, const int32_t *ref_q, int F_r,
                               const int32_t *group_of, int n_groups, same_score_features **out) {
    if (!mov || !out) return SAME_EINVAL;
    same_ctx *ctx = mov->ctx;
    *out = nullptr;
    REQUIRE(ctx, ref && ref->ctx->device == ctx->device);
    SAME_TRY(check_columns(ctx, "same_score_features_create", mov_q, mov->n, F_m, ref_q, ref->n, F_r, group_of, n_groups));
    SAME_TRY(same_use(ctx));
    same_score_features *f = new (std::nothrow) same_score_features();
    if (!f) return SAME_ENOMEM;
    f->ctx = ctx;
    f->mov = mov;
    f->ref = ref;
    f->F_m = F_m;
    f->F_r = F_r;
    f->n_groups = n_groups;
    *out = f;                                     // freed by the caller's destroy on any failure below
    SAME_TRY(upload(ctx, &f->mov_q, mov_q, (size_t)(mov->n * F_m)));
    SAME_TRY(upload(ctx, &f->ref_q, ref_q, (size_t)(ref->n * F_r)));
    SAME_TRY(upload(ctx, &f->group_of, group_of, (size_t)mov->n));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SAME_OK;
}

void same_score_features_destroy(same_score_features *f) {
    if (!f) return;
    (void)hipSetDevice(f->ctx->device);
    (void)hipDeviceSynchronize();                 // calls of other contexts may still be reading it
    if (f->mov_q) (void)hipFree(f->mov_q);
    if (f->ref_q) (void)hipFree(f->ref_q);
    if (f->group_of) (void)hipFree(f->group_of);
    delete f;
}

int same_feature_zone_create(const same_score_features *feats, const uint8_t *mov_flags, const uint8_t *ref_flags, const double *d2_edges,
                             int n_edges, same_feature_zone **out) {
    if (!feats || !out) return SAME_EINVAL;
    same_ctx *ctx = feats->ctx;
    *out = nullptr;
    SAME_TRY(check_edges(ctx, d2_edges, n_edges));
    SAME_TRY(same_use(ctx));
    same_feature_zone *z = new (std::nothrow) same_feature_zone();
    if (!z) return SAME_ENOMEM;
    z->ctx = ctx;
    z->feats = feats;
    z->B = n_edges - 1;
    *out = z;                                     // freed by the caller's destroy on any failure below
    SAME_TRY(upload(ctx, &z->mov_flags, mov_flags, (size_t)feats->mov->n));
    SAME_TRY(upload(ctx, &z->ref_flags, ref_flags, (size_t)feats->ref->n));
    SAME_TRY(upload(ctx, &z->edges, d2_edges, (size_t)n_edges));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SAME_OK;
}

void same_feature_zone_destroy(same_feature_zone *z) {
    if (!z) return;
    (void)hipSetDevice(z->ctx->device);
    (void)hipDeviceSynchronize();                 // calls of other contexts may still be reading it
    if (z->mov_flags) (void)hipFree(z->mov_flags);
    if (z->ref_flags) (void)hipFree(z->ref_flags);
    if (z->edges) (void)hipFree(z->edges);
    delete z;
}

int same_merge_acc_score_features(same_merge_acc *a, const same_section *mov, const same_section *ref, const same_score_features *feats,
                                  const same_feature_zone *zone, int64_t *out, int64_t out_words, double *out_d2) {
    if (!a) return SAME_EINVAL;
    same_ctx *ctx = a->ctx;
    REQUIRE(ctx, out);
    SAME_TRY(require_score_args(ctx, a, mov, ref, nullptr, 0.0));
    REQUIRE(ctx, feats && feats->mov == mov && feats->ref == ref && feats->ctx->device == ctx->device);
    REQUIRE(ctx, !zone || zone->feats == feats);
    FeatureLayout lo;
    lo.G = feats->n_groups;
    lo.F = feats->F_m + feats->F_r;
    lo.B = zone ? zone->B : 0;
    REQUIRE(ctx, out_words >= lo.out_words());
    SAME_TRY(same_use(ctx));
    const int64_t n = a->n_final, words = lo.words();
    const int G = lo.G, F = lo.F, B = lo.B;
    std::vector<unsigned long long> h((size_t)words, 0ull);
    unsigned long long zt[ZONE_TOTALS] = {};
    bool d2_copied = false;
    if (n > 0) {
        WorkSets &fs = a->feature_sets;
        if (!fs.fits(words)) {
            InDoubt laying(fs);
            SAME_TRY(lay_over(ctx, a->feature, a->fw, words));
            SAME_FILL(ctx, a->feature.p, 0, a->fw.bytes);
            fs.laid_anew(words);
        }
        const int64_t z_rows = std::max<int64_t>(std::max(n, mov->n), 1);
        ZoneWork zw;
        if (zone) {
            WorkSets &zs = a->zone_sets;
            if (!zs.fits(z_rows)) {
                InDoubt laying(zs);
                SAME_TRY(lay_over(ctx, a->zone, zw, z_rows));
                SAME_FILL(ctx, a->zone.p, 0, zw.zero_bytes);
                zs.laid_anew(z_rows);
            }
            Carver place(a->zone.p);
            lay(zw, place, a->zone_sets.laid);
        }
        InDoubt doubt(fs), doubt_zone(a->zone_sets);          // (the zone's: in doubt only where the call works in it)
        if (!zone) doubt_zone.sound();
        unsigned long long *bins = a->fw.bins + (size_t)fs.set * a->fw.cap, *next = a->fw.bins + (size_t)(fs.set ^ 1) * a->fw.cap;
        const FinalSource src{static_cast<const FinalRec *>(a->out.p), n, mov->n, ref->n};
        SAME_LAUNCH(ctx, feature_sums_kernel<FinalSource>, sums_grid(n, F, G + 1), dim3(NT), 0, src, feats->group_of, 0, G + 1, G, feats->mov_q,
                    feats->F_m, feats->ref_q, feats->F_r, bins + lo.rows(), bins + lo.sums(), bins + lo.bad(), next, fs.dirty);
        if (zone)                                 // (on its SAME_ERANGE both buffers stay in doubt: the next call lays them again)
            SAME_TRY(zone_phases(ctx, "same_merge_acc_score_features: final rows outside the sections (the accumulator's pass ran over other sections)",
                                 "same_merge_acc_score_features: a zone or subset pair's reference XY is not finite", src, zw, a->zone_sets.set,
                                 zone->mov_flags, zone->ref_flags, zone->edges, B, ref->xy, out_d2 != nullptr, feats->mov_q, feats->F_m,
                                 feats->ref_q, feats->F_r, bins + lo.bin_rows(), bins + lo.bin_sums(), zt));
        HIP_TRY(ctx, hipGetLastError());
        SAME_COPY(ctx, h.data(), bins, (size_t)words * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        if (zone && out_d2 && mov->n > 0) {
            SAME_COPY(ctx, out_d2, zw.d2, (size_t)mov->n * sizeof(double), hipMemcpyDeviceToHost);
            d2_copied = true;
        }
        SAME_WAIT(ctx);
        doubt.sound();
        fs.flip(words);
        if (zone) {
            doubt_zone.sound();
            a->zone_sets.flip();
        }
        if (h[(size_t)lo.bad()]) {
            ctx->err = "same_merge_acc_score_features: final rows outside the sections (the accumulator's pass ran over other sections)";
            return SAME_ERANGE;
        }
    }
    if (out_d2 && !d2_copied)
        for (int64_t i = 0; i < mov->n; ++i) out_d2[i] = std::nan("");
    for (int64_t q = 0; q < lo.out_words(); ++q) out[q] = (int64_t)h[(size_t)q];
    out[0] = n;
    out[1] = n - out[lo.rows() + G];
    out[2] = (int64_t)zt[Z_ZONE];
    out[3] = (int64_t)zt[Z_SUBSET];
    return SAME_OK;
}

}  // extern "C"
