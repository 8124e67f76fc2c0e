// Motion: per film sample the displacement from the first hit's surface point to where that point
// was before the frame's vertex updates, and its filtered plane (include/lumo_amd.h gives the
// definition operation by operation, DESIGN.md §4g "Motion" the design).
//
// A fragment of kernels.hip: included there after features.h, whose FeatSrc / feature_gather_plane
// and the film helpers it shares.  Per pass of a feature render that asks for motion, after
// k_closest_q (and k_features, when the feature planes are made too): k_motion turns each hit of
// S.hq into the sample's delta, k_motion_film (tiles of at most BLOCK pixels) or k_motion_gather
// (larger tiles) filters it into the plane.  Only kd-mesh triangles can move
// (lumo_scene_update_vertices protects everything else), so every other sample writes zeros and
// reads no vertex.

// Per-sample records of one task (lumo_debug_motion), laid out as FeatDump.
struct MotionDump {
    double *bary, *delta;
};

struct Motion {
    const double* vprev;  // the previous vertices (the present array before the first mark)
    double* dlt;          // per slot: the pass's delta (3)
    double* film_m;       // the filtered plane (4 doubles per slot, as Paths::film)
    MotionDump d;         // d.bary == nullptr: no dump
    int dump_p;           // pixels of the dumped task
};

// (bary.x A + bary.y B) + bary.z C of three vertices: tri_record_at's xi
__device__ __forceinline__ V3 motion_point(V3 bary, V3 A, V3 B, V3 Cv) { return bary.x * A + bary.y * B + bary.z * Cv; }

// One thread per queued camera path of the pass (queue `cur`, its closest hits in S.hq).  A hit on
// a kd mesh runs the accepted GEO test again on the object's local ray for e / det (the test is
// deterministic: object_record rebuilds the record the same way), forms the local point from the
// soup row and from the previous vertices of the same triangle, and carries the difference to
// world space as a direction.  72 B of vertices per moving hit beside the soup row the test reads.
template <int FX>
__global__ __launch_bounds__(BLOCK) void k_motion(DScene sc, Paths S, Motion M, QState cur, uint32_t pass) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= S.counts[CNT_CUR]) return;
    const HitQ hq = S.hq;
    const int slot = cur.I(QI_SLOT, q);
    V3 bary{0.0, 0.0, 0.0}, delta{0.0, 0.0, 0.0};
    if (hq.i[q] == 1) {  // an object: lights keep their vertices
        const lumo_object& ob = sc.objs[hq.i[hq.cap + q]];
        if (ob.type == LUMO_OBJ_KDMESH) {
            const int tri = hq.i[2 * hq.cap + q];
            RayX r = rayx(Ray{qv3(cur, QD_O, q), qv3(cur, QD_D, q)});
            if constexpr (FX != 0) {
                if (ob.xform >= 0) r = ray_local(sc.xforms[ob.xform], r);
            }
            const double* tv = sc.tv + TV_STRIDE * tri;
            Counters uncounted{0, 0, 0, 0};
            double t, delta_t;
            TriAcc acc;
            if (tri_test_at<true, true>(tv, r, 0.0, DINF, uncounted, t, acc, delta_t)) {
                bary = acc.e / acc.det;
                const int32_t* v = sc.tris[tri].v;
                const V3 xi = motion_point(bary, ld3(tv), ld3(tv + 3), ld3(tv + 6));
                const V3 xp = motion_point(bary, ld3(M.vprev + 3 * v[0]), ld3(M.vprev + 3 * v[1]), ld3(M.vprev + 3 * v[2]));
                delta = xp - xi;
                if constexpr (FX != 0) {
                    if (ob.xform >= 0) delta = xf_apply(sc.xforms[ob.xform].m, delta, 0.0);
                }
            }
        }
    }
    stv3(M.dlt, slot, delta);
    if (M.d.bary) {
        const size_t o = (size_t)pass * M.dump_p + S.pix[slot];
        stv3(M.d.bary, (int)o, bary);
        stv3(M.d.delta, (int)o, delta);
    }
}

// The plane of one pass for tasks of at most BLOCK pixels, one block per task: k_feature_film with
// one plane.  The tile's deltas, raster positions and validity and each sample's separable filter
// terms are staged in LDS (k_finish_film's expressions, so the weights are the beauty film's bit
// for bit), then gathered by film_gather_staged in the beauty film's order; filters wider than
// FILM_R go through film_gather_acc from LDS.
// LDS: 6 KiB values + 4 KiB raster + 1 KiB validity + 2 x 10 KiB terms + 2 KiB origins = 33 KiB.
__global__ __launch_bounds__(BLOCK) void k_motion_film(Paths S, Motion M, Tasks T, DCam cam, int t0) {
    __shared__ double l_val[3 * BLOCK];
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
            const V3 d = ldv3(M.dlt, s);
            for (int k = 0; k < 3; ++k) l_val[3 * j + k] = (&d.x)[k];
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
    double acc[4];
    for (int i = 0; i < 4; ++i) acc[i] = M.film_m[4 * s + i];
    if (pre)
        film_gather_staged(acc, T.t[ti], j, l_val, l_ox, l_oy, FilmTerms{l_wx, l_wy, r});
    else
        film_gather_acc(acc, T.t[ti], cam, j, LdsSrc{l_val, l_ras, l_ok});
    for (int i = 0; i < 4; ++i) M.film_m[4 * s + i] = acc[i];
}

// Tiles of any size: features.h' per-slot gather over the deltas.
__global__ __launch_bounds__(BLOCK) void k_motion_gather(Paths S, Motion M, Tasks T, DCam cam, int n) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= n) return;
    const int ti = S.task[s];
    feature_gather_plane(M.film_m, T.t[ti], cam, s, S.pix[s], FeatSrc{S, M.dlt, T.first[ti], false});
}
