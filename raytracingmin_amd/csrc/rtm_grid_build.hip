// rtm_grid_build.hip — rtm_scene_create_device (include/rtm.h): a scene object made from a DEVICE sphere array without the
// array, or anything of its size, travelling to the host; and rtm_debug_scene_grid (include/rtm_debug.h), which reads a scene's
// grid back.  The kernels are in rtm_grid_build_kernel.h; the scalar arithmetic of a build and the per-sphere expressions are
// the host builder's own (rtm_scene_facts.h: make_grid's; rtm_grid_exprs.h), so the tables are the ones make_grid makes, bit for bit.
// NOT a translation unit of its own: rtm_scene is private to rtm_kernels.hip, which includes this file at its end.
//
// The stages, all on the caller's stream ("Building the grid on the device"):
//   1  classification rounds: one reduction over the spheres per round (grid_round_kernel + its fold), the host turns the
//      box into the round's h and t_ok (grid_round_scalars) — 120 bytes down, two doubles up per round, at most five times
//   2  the padded box of the small spheres comes with the last round's reduction; the header is made on the host
//   3  per-sphere cell counts, an exclusive scan (rocPRIM: rtm_grid_prims.hip), the total comes back for the 32-bit guard and the allocation
//   4  (cell << 32 | sphere) keys written at the scanned offsets, sorted (rocPRIM radix sort over the bits in use):
//      ascending cell, ascending sphere within a cell — the host's counting-sort order
//   5  a cell's range by two binary searches in the sorted keys     6  the records     7  the big list by a scan of the flags
//   8  grid_far_bounces on the host from the big spheres' rows (at most kGridMaxBig of 40 bytes)
#include "rtm_grid_prims.h"

namespace rtm {

namespace {
unsigned grid_blocks(size_t items) { return (unsigned)((items + kGridBuildBlock - 1) / kGridBuildBlock); }

// One classification round: reduce, fold, bring the 120 bytes back.
int grid_round(const double4* geom, size_t n, unsigned* flags, int classify, double h, double t_ok, GridRound* partial,
               GridRound* out_dev, GridRound* out, hipStream_t stream) {
    const unsigned blocks = std::min<unsigned>(grid_blocks(n), (unsigned)kGridRoundMaxBlocks);
    grid_round_kernel<<<blocks, kGridBuildBlock, 0, stream>>>(geom, (unsigned)n, flags, classify, h, t_ok, partial);
    grid_round_fold_kernel<<<1, kGridBuildBlock, 0, stream>>>(partial, blocks, out_dev);
    RTM_HIP_CHECK(hipGetLastError());
    RTM_HIP_CHECK(hipMemcpyAsync(out, out_dev, sizeof *out, hipMemcpyDeviceToHost, stream));
    RTM_HIP_CHECK(hipStreamSynchronize(stream));
    return RTM_OK;
}

// The grid of sc's geometry rows, built on `stream`; a scene that gets no grid keeps sc.grid empty (not an error): the
// device form of build_scene_grid(make_grid(...)).
int build_scene_grid_device(rtm_scene& sc, size_t n, int device, hipStream_t stream) {
    const double lambda = grid_cells_per_sphere();
    if (n < kGridMinSpheres || n >= (1u << 29) || !(lambda > 0.0)) return RTM_OK;
    const double4* geom = sc.geom.as<double4>();
    DevMem block;  // the scene's grid; declared first, so that on every return it goes after the stream has been waited for
    struct StreamWait {
        hipStream_t stream;
        ~StreamWait() {
            (void)hipStreamSynchronize(stream);
            (void)hipGetLastError();
        }
    } wait_on_return{stream};
    AsyncMem flags, partial, round_dev;
    int rc = flags.alloc(n * sizeof(unsigned), stream);
    if (rc == RTM_OK) rc = partial.alloc((size_t)kGridRoundMaxBlocks * sizeof(GridRound), stream);
    if (rc == RTM_OK) rc = round_dev.alloc(sizeof(GridRound), stream);
    if (rc != RTM_OK) return rc;

    // ---- 1, 2: make_grid's loop of at most 4 rounds; `r` always holds the boxes of the spheres the last kernel left small
    GridRound r;
    if ((rc = grid_round(geom, n, flags.as<unsigned>(), 0, 0.0, 0.0, partial.as<GridRound>(), round_dev.as<GridRound>(), &r, stream)) != RTM_OK)
        return rc;
    if (r.bad != 0 || r.n_small < kGridMinSpheres) return RTM_OK;
    double h = 0.0, t_ok = 0.0;
    for (int round = 0; round < 4; ++round) {
        if (!grid_round_scalars(r.lo, r.hi, (size_t)r.n_small, lambda, h, t_ok)) return RTM_OK;
        if ((rc = grid_round(geom, n, flags.as<unsigned>(), 1, h, t_ok, partial.as<GridRound>(), round_dev.as<GridRound>(), &r, stream)) != RTM_OK)
            return rc;
        if (r.n_small < kGridMinSpheres) return RTM_OK;
        if (!r.changed && round > 0) break;
    }
    const size_t n_big = n - (size_t)r.n_small;
    if (n_big > (size_t)kGridMaxBig) return RTM_OK;
    GridHeader H;
    size_t cells = 0;
    if (!grid_header_from_box(r.plo, r.phi, h, t_ok, n, n_big, H, &cells)) return RTM_OK;
    const GridBuildDims D = grid_build_dims(H);

    // ---- 3: counts, their exclusive scan, the total
    AsyncMem count, offset, scan_tmp;
    if ((rc = count.alloc((n + 1) * sizeof(unsigned), stream)) != RTM_OK) return rc;
    if ((rc = offset.alloc((n + 1) * sizeof(unsigned long long), stream)) != RTM_OK) return rc;
    grid_count_kernel<<<grid_blocks(n + 1), kGridBuildBlock, 0, stream>>>(geom, (unsigned)n, flags.as<unsigned>(), D, t_ok, count.as<unsigned>());
    RTM_HIP_CHECK(hipGetLastError());
    size_t tmp_counts = 0, tmp_flags = 0;
    RTM_HIP_CHECK(grid_scan_counts(nullptr, tmp_counts, count.as<unsigned>(), offset.as<unsigned long long>(), n + 1, stream));
    RTM_HIP_CHECK(grid_scan_flags(nullptr, tmp_flags, flags.as<unsigned>(), count.as<unsigned>(), n, stream));
    if ((rc = scan_tmp.alloc(std::max(tmp_counts, tmp_flags), stream)) != RTM_OK) return rc;
    RTM_HIP_CHECK(grid_scan_counts(scan_tmp.p, tmp_counts, count.as<unsigned>(), offset.as<unsigned long long>(), n + 1, stream));
    unsigned long long refs = 0;
    RTM_HIP_CHECK(hipMemcpyAsync(&refs, offset.as<unsigned long long>() + n, sizeof refs, hipMemcpyDeviceToHost, stream));
    RTM_HIP_CHECK(hipStreamSynchronize(stream));
    if (refs > 0xFFFFFF00ull) return RTM_OK;
    const size_t n_recs = refs ? (size_t)refs : 1;

    // ---- the scene's block, laid out as build_scene_grid lays it out; the kernels below write straight into it
    const GridLayout lay = grid_layout(cells, n_recs, n_big);
    if ((rc = block.alloc_pooled(lay.bytes, device)) != RTM_OK) return rc;
    unsigned char* base = block.as<unsigned char>();
    H.cell_range = reinterpret_cast<const uint2*>(base + lay.off_cs);
    H.recs = reinterpret_cast<const double4*>(base + lay.off_items);
    H.n_recs = (unsigned)n_recs;
    H.big = reinterpret_cast<const int*>(base + lay.off_big);
    RTM_HIP_CHECK(hipMemcpyAsync(base, &H, sizeof H, hipMemcpyHostToDevice, stream));

    // ---- 4: the keys, sorted
    AsyncMem keys_in, keys_out, sort_tmp;
    if ((rc = keys_in.alloc(n_recs * sizeof(unsigned long long), stream)) != RTM_OK) return rc;
    if ((rc = keys_out.alloc(n_recs * sizeof(unsigned long long), stream)) != RTM_OK) return rc;
    if (refs) {
        grid_fill_kernel<<<grid_blocks(n), kGridBuildBlock, 0, stream>>>(geom, (unsigned)n, flags.as<unsigned>(), D, t_ok,
                                                                        offset.as<unsigned long long>(), refs,
                                                                        keys_in.as<unsigned long long>());
        RTM_HIP_CHECK(hipGetLastError());
        unsigned cell_bits = 1;
        while (cell_bits < 32 && ((size_t)1 << cell_bits) < cells) ++cell_bits;
        size_t tmp_sort = 0;
        RTM_HIP_CHECK(grid_sort_keys(nullptr, tmp_sort, keys_in.as<unsigned long long>(), keys_out.as<unsigned long long>(), (size_t)refs,
                                     32u + cell_bits, stream));
        if ((rc = sort_tmp.alloc(tmp_sort, stream)) != RTM_OK) return rc;
        RTM_HIP_CHECK(grid_sort_keys(sort_tmp.p, tmp_sort, keys_in.as<unsigned long long>(), keys_out.as<unsigned long long>(), (size_t)refs,
                                     32u + cell_bits, stream));
    }
    // ---- 5, 6: the cells' ranges and the records
    grid_ranges_kernel<<<grid_blocks(cells), kGridBuildBlock, 0, stream>>>(keys_out.as<unsigned long long>(), (unsigned)refs,
                                                                          (unsigned long long)cells,
                                                                          reinterpret_cast<uint2*>(base + lay.off_cs));
    grid_records_kernel<<<grid_blocks(n_recs), kGridBuildBlock, 0, stream>>>(geom, (unsigned)n, keys_out.as<unsigned long long>(),
                                                                            (unsigned)refs, (unsigned)n_recs,
                                                                            reinterpret_cast<double4*>(base + lay.off_items));
    RTM_HIP_CHECK(hipGetLastError());

    // ---- 7, 8: the big list, its rows back for the decision
    std::vector<int> big(n_big);
    std::vector<double> big_rows(n_big * 5);
    AsyncMem rows_dev;
    if (n_big) {
        if ((rc = rows_dev.alloc(n_big * 5 * sizeof(double), stream)) != RTM_OK) return rc;
        // (count's values are spent: it takes the flags' scan)
        RTM_HIP_CHECK(grid_scan_flags(scan_tmp.p, tmp_flags, flags.as<unsigned>(), count.as<unsigned>(), n, stream));
        grid_big_kernel<<<grid_blocks(n), kGridBuildBlock, 0, stream>>>(geom, sc.mat.as<double>(), (unsigned)n, flags.as<unsigned>(),
                                                                       count.as<unsigned>(), (unsigned)n_big,
                                                                       reinterpret_cast<int*>(base + lay.off_big), rows_dev.as<double>());
        RTM_HIP_CHECK(hipGetLastError());
        RTM_HIP_CHECK(hipMemcpyAsync(big.data(), base + lay.off_big, n_big * sizeof(int), hipMemcpyDeviceToHost, stream));
        RTM_HIP_CHECK(hipMemcpyAsync(big_rows.data(), rows_dev.p, big_rows.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    }
    RTM_HIP_CHECK(hipStreamSynchronize(stream));  // the tables are resident; H and the vectors may go
    const int far = grid_far_bounces_of(H, big.data(), n_big, nullptr, [&](size_t j, int) { return &big_rows[j * 5]; },
                                        [&](size_t j, int) { return big_rows[j * 5 + 4] > 0.0; });
    if (far < 0) return RTM_OK;  // (a plane's row: a sphere array has none)
    sc.grid_far_bounces = far != 0;
    sc.grid.p = block.p;
    sc.grid.pooled_device = block.pooled_device;
    block.p = nullptr;
    block.pooled_device = -1;
    sc.grid_hdr = H;
    sc.grid_cells = cells;
    sc.grid_refs = n_recs;
    sc.grid_big = n_big;
    return RTM_OK;
}
}  // namespace

int scene_create_device(const rtm_sphere* sp_dev, size_t n, int device, void* stream_v, rtm_scene** out) {
    if (!out) return invalid("null out_scene");
    if (!sp_dev && n) return invalid("null spheres_dev");
    if (n > 0x7FFFFFFFull) return invalid("scene too large");
    if (device < 0) return invalid("negative device");
    *out = nullptr;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    std::unique_ptr<rtm_scene> sc(new rtm_scene);
    int rc = scene_tables_device(*sc, sp_dev, n, device, stream);
    if (rc == RTM_OK) rc = build_scene_grid_device(*sc, n, device, stream);
    if (rc != RTM_OK) {
        (void)hipStreamSynchronize(stream);  // nothing queued here may outlive the tables it writes
        (void)hipGetLastError();
        return rc;
    }
    *out = sc.release();
    return RTM_OK;
}

// rtm_debug_scene_grid: a scene's grid as the device holds it, in grid_build_host's format
int scene_grid_probe(const rtm_scene* sc, uint64_t* info, uint32_t* ranges, size_t ranges_cap, uint32_t* items, size_t items_cap,
                     int32_t* big, size_t big_cap, uint64_t* extra) {
    if (!sc || !info) return invalid("null scene or info");
    if (!sc->grid.p) return unsupported("this scene has no grid");
    DeviceGuard guard;
    RTM_HIP_CHECK(hipSetDevice(sc->device));
    const GridHeader& H = sc->grid_hdr;
    const size_t cells = sc->grid_cells, n_recs = sc->grid_refs, n_big = sc->grid_big;
    std::vector<unsigned> rg(cells * 2);
    RTM_HIP_CHECK(hipMemcpy(rg.data(), H.cell_range, rg.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    const size_t refs = cells ? rg[cells * 2 - 1] : 0;  // (the one dummy record of a grid without entries is not an entry)
    info[0] = cells;
    info[1] = refs;
    info[2] = n_big;
    for (int k = 0; k < 3; ++k) info[3 + k] = (uint64_t)H.dim[k];
    const double d[6] = {H.lo[0], H.lo[1], H.lo[2], H.h, std::sqrt(H.reach2), H.t_ok};
    std::memcpy(info + 6, d, sizeof d);
    if (extra) extra[1] = sc->grid_far_bounces ? 1u : 0u;
    if ((ranges && ranges_cap < cells * 2) || (items && items_cap < refs) || (big && big_cap < n_big)) return RTM_ERR_CAPACITY;
    if (ranges) std::memcpy(ranges, rg.data(), rg.size() * sizeof(unsigned));
    if (big && n_big) RTM_HIP_CHECK(hipMemcpy(big, H.big, n_big * sizeof(int), hipMemcpyDeviceToHost));
    if (items || extra) {
        std::vector<double> recs(n_recs * 4), geom(sc->n * 4);
        RTM_HIP_CHECK(hipMemcpy(recs.data(), H.recs, recs.size() * sizeof(double), hipMemcpyDeviceToHost));
        RTM_HIP_CHECK(hipMemcpy(geom.data(), sc->geom.p, geom.size() * sizeof(double), hipMemcpyDeviceToHost));
        uint64_t wrong = 0;
        for (size_t k = 0; k < n_recs; ++k) {
            unsigned long long wbits;
            std::memcpy(&wbits, &recs[k * 4 + 3], sizeof wbits);
            const size_t i = (size_t)(wbits & 0x1FFFFFFFull);
            if (items && k < refs) items[k] = (uint32_t)i;
            bool same = i < sc->n && std::memcmp(&recs[k * 4], &geom[i * 4], 3 * sizeof(double)) == 0;
            if (same) {
                unsigned long long gbits;
                std::memcpy(&gbits, &geom[i * 4 + 3], sizeof gbits);
                same = wbits == (gbits | (unsigned long long)i);
            }
            wrong += same ? 0u : 1u;
        }
        if (extra) extra[0] = wrong;
    }
    return RTM_OK;
}

}  // namespace rtm
