// Feature buffers: the first hit's albedo, shading normal and depth of every film sample, as
// per-sample records and as filtered planes aligned with the beauty film.
//
// A fragment of kernels.hip: included there inside its anonymous namespace, after the film helpers
// it shares with the beauty film (sample_rgb, gauss, FilmTerms, film_gather_acc,
// film_gather_staged, LdsSrc).  Per pass: k_camera<true> queues the camera paths, k_closest_q
// walks them, k_features turns each hit into the sample's features, k_feature_film (tiles of at
// most BLOCK pixels) or k_feature_gather (larger tiles) filters them into the three planes.
// Nothing here is taken by the beauty kernels: the planes travel in Feat.

// Per-sample records of one task (lumo_debug_features), pass-major, pixels in raster order.
struct FeatDump {
    int32_t *kind, *object, *prim, *material, *backface;
    double *t, *p, *ng, *ns, *n, *uv, *albedo, *albedo_rgb, *raster, *lam;
};

// Per slot: the pass's features (albedo RGB, oriented shading normal, (t, hit)) and the three
// filtered planes (4 doubles each, as Paths::film).
struct Feat {
    double *alb, *nrm, *dep;
    double *film_a, *film_n, *film_d;
    FeatDump d;  // d.kind == nullptr: no dump
    int dump_p;  // pixels of the dumped task
};

// The first-hit albedo at the sample's wavelengths: kd of the diffuse materials, ks of a
// conductor, tf of a dielectric, 1 for a light, 0 for Blank.
template <int FX>
__device__ __forceinline__ DColor feature_albedo(const DScene& sc, const lumo_material& m, V2 uv, const double* L) {
    switch (m.kind) {
        case LUMO_MAT_LAMBERTIAN:
        case LUMO_MAT_MF_DIFFUSE: return mat_kd<FX>(sc, m, uv, L);
        case LUMO_MAT_MF_CONDUCTOR: return mat_ks<FX>(sc, m, uv, L);
        case LUMO_MAT_MF_DIELECTRIC: return mat_tf<FX>(sc, m, uv, L);
        case LUMO_MAT_LIGHT: return cfill(1.0);
        default: return cfill(0.0);
    }
}

// One thread per queued camera path of the pass (queue `cur`, its closest hits in S.hq): the hit
// record of the first hit (the oracle's bounce-0 record; nothing is followed through mirrors or
// glass) and from it the sample's features, written per slot; a miss writes zeros.
template <int FX>
__global__ __launch_bounds__(BLOCK) void k_features(DScene sc, Paths S, Feat F, DCam cam, QState cur, uint32_t pass) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= S.counts[CNT_CUR]) return;
    const HitQ hq = S.hq;
    const int slot = cur.I(QI_SLOT, q);
    const Ray ro{qv3(cur, QD_O, q), qv3(cur, QD_D, q)};
    double L[NS];
    for (int i = 0; i < NS; ++i) L[i] = cur.D(QD_L + i, q);
    const int kind = hq.i[q];
    const int obj = kind ? hq.i[hq.cap + q] : -1, tri = kind ? hq.i[2 * hq.cap + q] : -1;
    DHit ho;
    ho.t = 0.0, ho.material = -1, ho.backface = false;
    ho.p = ho.err = ho.ns = ho.ng = V3{0.0, 0.0, 0.0};
    ho.uv = V2{0.0, 0.0};
    V3 ns{0.0, 0.0, 0.0}, n{0.0, 0.0, 0.0}, rgb{0.0, 0.0, 0.0};
    DColor albedo = cfill(0.0);
    if (kind != 0) {
        hit_record<FX>(sc, HitRef{hq.t[q], kind, obj, tri}, rayx(ro), ho);
        const lumo_material& m = sc.mats[ho.material];
        ns = mapped_ns<FX>(sc, m, ho);
        n = ho.backface ? -ns : ns;
        albedo = feature_albedo<FX>(sc, m, ho.uv, L);
        rgb = sample_rgb(sc, cam, albedo, L, LUMO_TONEMAP_NONE, 0.0);
    }
    stv3(F.alb, slot, rgb);
    stv3(F.nrm, slot, n);
    F.dep[2 * slot] = ho.t;
    F.dep[2 * slot + 1] = kind != 0 ? 1.0 : 0.0;
    const FeatDump& d = F.d;
    if (d.kind) {
        const size_t o = (size_t)pass * F.dump_p + S.pix[slot];
        d.kind[o] = kind;
        d.object[o] = obj;
        d.prim[o] = tri;
        d.material[o] = ho.material;
        d.backface[o] = ho.backface ? 1 : 0;
        d.t[o] = ho.t;
        stv3(d.p, (int)o, ho.p);
        stv3(d.ng, (int)o, ho.ng);
        stv3(d.ns, (int)o, ns);
        stv3(d.n, (int)o, n);
        d.uv[2 * o] = ho.uv.x;
        d.uv[2 * o + 1] = ho.uv.y;
        stc(d.albedo, (int)o, albedo);
        stv3(d.albedo_rgb, (int)o, rgb);
        d.raster[2 * o] = S.raster[2 * slot];
        d.raster[2 * o + 1] = S.raster[2 * slot + 1];
        for (int i = 0; i < NS; ++i) d.lam[4 * o + i] = L[i];
    }
}

// The depth plane's source value: (t hit, hit, 0), so that its channels gather to
// (sum w t hit, sum w hit, 0, sum w).
__device__ __forceinline__ V3 depth_value(const double* dep, int s) {
    const double t = dep[2 * s], hit = dep[2 * s + 1];
    return V3{t * hit, hit, 0.0};
}

// The three planes of one pass for tasks of at most BLOCK pixels, one block per task: the tile's
// samples staged in LDS, each sample's separable filter terms computed once (the staging of
// k_finish_film: same expressions, so the weights are the beauty film's bit for bit) and all three
// planes gathered with them by film_gather_staged, in the beauty film's order.  Wider filters than
// FILM_R go through film_gather_acc from LDS, as in k_finish_film.
// LDS: 3 x 6 KiB values + 4 KiB raster + 1 KiB validity + 2 x 10 KiB terms + 2 KiB origins = 45 KiB.
__global__ __launch_bounds__(BLOCK) void k_feature_film(Paths S, Feat F, Tasks T, DCam cam, int t0) {
    __shared__ double l_val[3][3 * BLOCK];  // albedo RGB, normal, (t hit, hit, 0)
    __shared__ double l_ras[2 * BLOCK];
    __shared__ uint32_t l_ok[BLOCK];
    __shared__ double l_wx[(2 * FILM_R + 1) * BLOCK], l_wy[(2 * FILM_R + 1) * BLOCK];
    __shared__ int l_ox[BLOCK], l_oy[BLOCK];
    const int ti = t0 + (int)blockIdx.x;
    const int first = T.first[ti];
    const int P = T.first[ti + 1] - first;
    const int j = threadIdx.x;
    const int s = first + j;
    const int r = (int)ceil(cam.fr - 0.5);
    const bool pre = r <= FILM_R;  // uniform
    if (j < P) {
        const bool ok = S.p_valid[s] != 0;
        l_ok[j] = ok ? 1u : 0u;
        l_ox[j] = l_oy[j] = INT_MIN / 4;
        if (ok) {
            const V3 a = ldv3(F.alb, s), n = ldv3(F.nrm, s), d = depth_value(F.dep, s);
            for (int k = 0; k < 3; ++k) {
                l_val[0][3 * j + k] = (&a.x)[k];
                l_val[1][3 * j + k] = (&n.x)[k];
                l_val[2][3 * j + k] = (&d.x)[k];
            }
            const double rx = S.raster[2 * s], ry = S.raster[2 * s + 1];
            l_ras[2 * j] = rx;
            l_ras[2 * j + 1] = ry;
            if (pre) {  // this sample's column / row terms, as k_finish_film stages them
                const double gr = gauss(cam.fr, cam.fsig);
                const int64_t px = rx > 0.0 ? (int64_t)floor(rx) : 0, py = ry > 0.0 ? (int64_t)floor(ry) : 0;
                l_ox[j] = (int)(px - r - (int64_t)T.t[ti].px_min[0]);
                l_oy[j] = (int)(py - r - (int64_t)T.t[ti].px_min[1]);
                for (int i = 0; i <= 2 * r; ++i) {
                    const double gx = (double)(px - r + i), gy = (double)(py - r + i);
                    l_wx[i * BLOCK + j] = rmax(gauss(rx - (0.5 + gx), cam.fsig) - gr, 0.0);
                    l_wy[i * BLOCK + j] = rmax(gauss(ry - (0.5 + gy), cam.fsig) - gr, 0.0);
                }
            }
        }
    }
    __syncthreads();
    if (j >= P) return;
    const FilmTerms terms{l_wx, l_wy, r};
    double* const film[3] = {F.film_a, F.film_n, F.film_d};
    for (int k = 0; k < 3; ++k) {
        double acc[4];
        for (int i = 0; i < 4; ++i) acc[i] = film[k][4 * s + i];
        if (pre)
            film_gather_staged(acc, T.t[ti], j, l_val[k], l_ox, l_oy, terms);
        else
            film_gather_acc(acc, T.t[ti], cam, j, LdsSrc{l_val[k], l_ras, l_ok});
        for (int i = 0; i < 4; ++i) film[k][4 * s + i] = acc[i];
    }
}

// Tiles of any size: the plain per-slot gather (k_film's), once per plane, sources from HBM.
struct FeatSrc {
    const Paths& S;
    const double* v;  // 3 per slot, or the (t, hit) pairs when `depth`
    int first;
    bool depth;
    __device__ bool valid(int k) const { return S.p_valid[first + k] != 0; }
    __device__ double rx(int k) const { return S.raster[2 * (first + k)]; }
    __device__ double ry(int k) const { return S.raster[2 * (first + k) + 1]; }
    __device__ V3 rgb(int k) const { return depth ? depth_value(v, first + k) : ldv3(v, first + k); }
};
__device__ __forceinline__ void feature_gather_plane(double* film, const lumo_tile_task& t, const DCam& cam, int s, int j,
                                                     const FeatSrc& src) {
    double acc[4] = {film[4 * s], film[4 * s + 1], film[4 * s + 2], film[4 * s + 3]};
    film_gather_acc(acc, t, cam, j, src);
    for (int i = 0; i < 4; ++i) film[4 * s + i] = acc[i];
}
__global__ __launch_bounds__(BLOCK) void k_feature_gather(Paths S, Feat F, Tasks T, DCam cam, int n) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= n) return;
    const int ti = S.task[s], first = T.first[ti], j = S.pix[s];
    feature_gather_plane(F.film_a, T.t[ti], cam, s, j, FeatSrc{S, F.alb, first, false});
    feature_gather_plane(F.film_n, T.t[ti], cam, s, j, FeatSrc{S, F.nrm, first, false});
    feature_gather_plane(F.film_d, T.t[ti], cam, s, j, FeatSrc{S, F.dep, first, true});
}
