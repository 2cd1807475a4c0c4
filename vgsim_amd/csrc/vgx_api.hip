// vgx_api.hip — host side of libvgx.so: the C ABI of include/vgx.h.
//
// Owns device memory (hipMalloc), one HIP stream and a pair of HIP events per engine; converts between
// the reference's dense host arrays (BirthDeathModel fields, src/_BirthDeath.pyx:47-68) and the engine's
// HBM layout (vgx_dev.h); does the parameter-only parts of UpdateAllRates (pyx:284-297, 340-344) and the
// first-call part of PrepareParameters (pyx:435-448) on the host, in the reference's operation order
// (this file is compiled with -ffp-contract=off as well); launches the kernels.
#include "vgx_engine.h"
#include "vgx_mutation_spectrum.h"   // (declares its launcher, vgxi_ms_spectrum, itself)
#include "vgx_introductions.h"       // (and vgxi_in_lineages)
#include "vgx_rng.h"

static std::string g_create_error;

extern "C" int vgx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int vgx_create(const vgx_dims *dims, int64_t n_replicates, int device, vgx_engine **out) {
    if (!dims || !out || n_replicates < 1) { g_create_error = "vgx_create: bad argument"; return VGX_ERR_ARG; }
    int64_t h = 1;
    for (int64_t s = 0; s < dims->sites; s++) h *= 4;
    if (dims->sites < 0 || dims->sites > 15 || dims->hapNum != h || dims->popNum < 1 || dims->susNum < 1) {
        g_create_error = "vgx_create: hapNum must equal 4^sites (sites <= 15), popNum >= 1, susNum >= 1";
        return VGX_ERR_ARG;
    }
    int n = 0;
    hipError_t he = hipGetDeviceCount(&n);
    if (he != hipSuccess || n == 0) {
        g_create_error = std::string("vgx_create: no HIP device available (") + hipGetErrorString(he) +
                         "); this engine has no CPU fallback";
        return VGX_ERR_HIP;
    }
    if (device < 0 || device >= n) { g_create_error = "vgx_create: device index out of range"; return VGX_ERR_ARG; }
    vgx_engine *e = new vgx_engine();
    e->d = *dims;
    e->R = n_replicates;
    e->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&e->stream) != hipSuccess ||
        hipEventCreate(&e->ev0) != hipSuccess || hipEventCreate(&e->ev1) != hipSuccess) {
        g_create_error = "vgx_create: could not create stream/events";
        delete e;
        return VGX_ERR_HIP;
    }
    e->seeds.assign((size_t)n_replicates, 0);
    *out = e;
    return VGX_OK;
}

extern "C" void vgx_destroy(vgx_engine *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    for (DevBuf *b : e->all)
        if (b->p) (void)hipFree(b->p);
    for (int i = 0; i < 2; i++) {
        if (e->pin[i]) (void)hipHostFree(e->pin[i]);
        if (e->pin_ev[i]) (void)hipEventDestroy(e->pin_ev[i]);
    }
    if (e->pin_tau) (void)hipHostFree(e->pin_tau);
    if (e->pin_tl) (void)hipHostFree(e->pin_tl);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

extern "C" const char *vgx_last_error(const vgx_engine *e) { return e ? e->err.c_str() : g_create_error.c_str(); }
extern "C" double vgx_last_kernel_ms(const vgx_engine *e) { return e ? (double)e->last_ms : 0.0; }
extern "C" int64_t vgx_last_kernel_launches(const vgx_engine *e) { return e ? e->last_launches : 0; }
extern "C" int vgx_last_direct_kernel(const vgx_engine *e) {
    if (!e) return 0;
    return e->last_kernel == VGX_K_QUADF ? VGX_K_QUAD : (int)e->last_kernel;
}
extern "C" int64_t vgx_device_bytes(const vgx_engine *e) { return e ? (int64_t)e->dev_bytes : 0; }

extern "C" int vgx_set_seeds(vgx_engine *e, const int64_t *seeds) {
    if (!e || !seeds) return VGX_ERR_ARG;
    for (int64_t r = 0; r < e->R; r++) {
        if (seeds[r] < 0) return fail(e, VGX_ERR_ARG, "vgx_set_seeds: seeds must be >= 0");
        e->seeds[(size_t)r] = seeds[r];
    }
    return VGX_OK;
}

// The tables VgxDevParams points to that are derived from one vgx_params: the classes of identical per-haplotype rate rows and the
// parameter-only parts of UpdateAllRates.  vgx_set_params installs one of them; vgx_set_param_sets builds one per set.
struct ParamTables {
    std::vector<int32_t> cls, c_bidx, c_stype;
    std::vector<double> c_d, c_s, c_tm, cb_b, cb_sig, suscepCumul, mig, actualSizes;
    double maxEffectiveBirth = 0.0;
};

// `who` opens the message of a refusal ("vgx_set_params", "vgx_set_param_sets: set 3")
static int build_param_tables(const vgx_dims &d, const vgx_params *p, const std::string &who, ParamTables &t, std::string &err) {
    const int64_t H = d.hapNum, P = d.popNum, S = d.susNum, sites = d.sites;
    if (!p->bRate || !p->dRate || !p->sRate || !p->susceptibility || !p->suscType || !p->suscepTransition ||
        !p->sizes || !p->contactDensityBeforeLockdown || !p->contactDensityAfterLockdown || !p->startLD ||
        !p->endLD || !p->samplingMultiplier || !p->migrationRates || (sites > 0 && (!p->mRate || !p->hapMutType))) {
        err = who + ": null parameter array";
        return VGX_ERR_ARG;
    }
    for (int64_t h = 0; h < H; h++)
        if (p->suscType[h] < 0 || p->suscType[h] >= S) { err = who + ": suscType out of range"; return VGX_ERR_ARG; }

    // ---- classes of identical per-haplotype rate rows ----
    std::vector<double> tm((size_t)H);
    for (int64_t h = 0; h < H; h++) {  // tmRate, pyx:306-308
        double tt = 0;
        for (int64_t s = 0; s < sites; s++) tt += p->mRate[h * sites + s];
        tm[(size_t)h] = tt;
    }
    std::unordered_map<std::string, int> fullmap, birthmap;
    std::vector<double> &c_d = t.c_d, &c_s = t.c_s, &c_tm = t.c_tm, &cb_b = t.cb_b, &cb_sig = t.cb_sig;
    std::vector<int32_t> &c_bidx = t.c_bidx, &c_stype = t.c_stype;
    c_d.clear(); c_s.clear(); c_tm.clear(); cb_b.clear(); cb_sig.clear(); c_bidx.clear(); c_stype.clear();
    t.cls.assign((size_t)H, 0);
    std::string key;
    for (int64_t h = 0; h < H; h++) {
        key.assign((const char *)&p->bRate[h], 8);
        key.append((const char *)&p->susceptibility[h * S], (size_t)S * 8);
        auto bi = birthmap.find(key);
        int cb;
        if (bi == birthmap.end()) {
            cb = (int)cb_b.size();
            birthmap.emplace(key, cb);
            cb_b.push_back(p->bRate[h]);
            for (int64_t s = 0; s < S; s++) cb_sig.push_back(p->susceptibility[h * S + s]);
        } else {
            cb = bi->second;
        }
        key.append((const char *)&p->dRate[h], 8);
        key.append((const char *)&p->sRate[h], 8);
        key.append((const char *)&tm[(size_t)h], 8);
        key.append((const char *)&p->suscType[h], 8);
        auto fi = fullmap.find(key);
        int c;
        if (fi == fullmap.end()) {
            c = (int)c_d.size();
            fullmap.emplace(key, c);
            c_d.push_back(p->dRate[h]);
            c_s.push_back(p->sRate[h]);
            c_tm.push_back(tm[(size_t)h]);
            c_bidx.push_back(cb);
            c_stype.push_back((int32_t)p->suscType[h]);
            if (c_d.size() > VGX_MAX_CLASSES) {
                err = who + ": more than " + std::to_string(VGX_MAX_CLASSES) +
                      " distinct per-haplotype rate rows (bRate, susceptibility, dRate, sRate, sum of mRate, suscType)";
                return VGX_ERR_CLASSES;
            }
        } else {
            c = fi->second;
        }
        t.cls[(size_t)h] = c;
    }

    // ---- parameter-only parts of UpdateAllRates, in the reference's order ----
    t.suscepCumul.assign((size_t)S, 0.0);
    for (int64_t s1 = 0; s1 < S; s1++) {  // pyx:284-287
        double v = 0;
        for (int64_t s2 = 0; s2 < S; s2++) v += p->suscepTransition[s1 * S + s2];
        t.suscepCumul[(size_t)s1] = v;
    }
    t.mig.assign(p->migrationRates, p->migrationRates + P * P);
    t.actualSizes.assign((size_t)P, 0.0);
    for (int64_t p1 = 0; p1 < P; p1++) {  // pyx:289-297
        t.mig[(size_t)(p1 * P + p1)] = 1.0;
        double a = 0.0;
        for (int64_t p2 = 0; p2 < P; p2++) {
            if (p1 == p2) continue;
            t.mig[(size_t)(p1 * P + p1)] -= t.mig[(size_t)(p1 * P + p2)];
            a += t.mig[(size_t)(p2 * P + p1)] * (double)p->sizes[p2];
        }
        // NB: the reference reads migrationRates[pn2, pn1] for pn2 != pn1 only, so the not-yet-rewritten
        // diagonals of later rows never enter (pyx:296)
        a += t.mig[(size_t)(p1 * P + p1)] * (double)p->sizes[p1];
        t.actualSizes[(size_t)p1] = a;
    }
    t.maxEffectiveBirth = 0.0;  // pyx:340-344
    for (int64_t h = 0; h < H; h++)
        for (int64_t s = 0; s < S; s++) {
            double v = p->bRate[h] * p->susceptibility[h * S + s];
            if (v > t.maxEffectiveBirth) t.maxEffectiveBirth = v;
        }
    return VGX_OK;
}

// What the start of a tau call reads of one parameter set beyond its device block: which rate classes have any positive rate, and
// the table of the uniform mutation model (every haplotype with the same mRate / hapMutType rows)
static void tau_set_tables(const vgx_dims &d, const vgx_params *p, const ParamTables &t, TauSetTables &out) {
    const int64_t H = d.hapNum, sites = d.sites;
    out.cls = t.cls;
    out.suscepCumul = t.suscepCumul;
    out.class_pos.assign(t.c_d.size(), 0);
    for (size_t c = 0; c < t.c_d.size(); c++)
        out.class_pos[c] = (t.c_d[c] > 0.0 || t.c_s[c] > 0.0 || t.c_tm[c] > 0.0 || t.cb_b[(size_t)t.c_bidx[c]] > 0.0) ? 1 : 0;
    out.mut_uniform = true;
    for (int64_t h = 1; h < H && out.mut_uniform; h++)
        if (memcmp(p->mRate + h * sites, p->mRate, (size_t)sites * 8) != 0 ||
            memcmp(p->hapMutType + h * sites * 3, p->hapMutType, (size_t)sites * 24) != 0)
            out.mut_uniform = false;
    for (int64_t s2 = 0; s2 < sites && s2 < 16; s2++) {
        const double *hm = p->hapMutType + s2 * 3;
        for (int i = 0; i < 3; i++) out.mutp[s2][i] = p->mRate[s2] * hm[i] / (hm[0] + hm[1] + hm[2]);
    }
}

extern "C" int vgx_set_params(vgx_engine *e, const vgx_params *p) {
    if (!e || !p) return VGX_ERR_ARG;
    HIPCHECK(e, hipSetDevice(e->device));
    const int64_t H = e->d.hapNum, P = e->d.popNum, S = e->d.susNum, sites = e->d.sites;
    ParamTables t;
    {
        std::string msg;
        const int rc = build_param_tables(e->d, p, "vgx_set_params", t, msg);
        if (rc) return fail(e, rc, msg);
    }
    const std::vector<double> &c_d = t.c_d, &c_s = t.c_s, &c_tm = t.c_tm, &cb_b = t.cb_b, &cb_sig = t.cb_sig;
    const std::vector<int32_t> &c_bidx = t.c_bidx, &c_stype = t.c_stype;
    e->cls = t.cls;
    e->C = (int)c_d.size();
    e->CB = (int)cb_b.size();
    {   // BirthRate (pyx:382-392) per birth class as a program of chain segments: the groups with a non-zero susceptibility in
        // order, common prefixes (group, susceptibility) of different classes shared (vgx_quadg.hip)
        e->h_seg_par.clear(); e->h_seg_sn.clear(); e->h_seg_sig.clear();
        e->h_cb_seg.assign(cb_b.size(), -1);
        std::unordered_map<std::string, int> segmap;
        for (size_t cb = 0; cb < cb_b.size(); cb++) {
            int cur = -1;
            for (int64_t sn = 0; sn < S; sn++) {
                const double sg = cb_sig[cb * (size_t)S + (size_t)sn];
                if (sg == 0.0) continue;
                std::string k((const char *)&cur, sizeof(cur));
                k.append((const char *)&sn, sizeof(sn));
                k.append((const char *)&sg, sizeof(sg));
                auto it = segmap.find(k);
                if (it == segmap.end()) {
                    const int id = (int)e->h_seg_par.size();
                    segmap.emplace(k, id);
                    e->h_seg_par.push_back(cur); e->h_seg_sn.push_back((int32_t)sn); e->h_seg_sig.push_back(sg);
                    cur = id;
                } else {
                    cur = it->second;
                }
            }
            e->h_cb_seg[cb] = cur;
        }
    }
    {   // the single-trajectory kernel runs that program two chains at a time (vgx_solo.h): a segment is ready when its parent is done,
        // the sum of the migration rates (-2) from the start
        e->h_so_pass.assign(4 * VGX_SOLO_MAX_PASS, -1);
        const int ns = (int)e->h_seg_par.size();
        for (int with_mig = 0; with_mig < 2; with_mig++) {
            std::vector<char> done((size_t)ns, 0);
            bool mig_done = !with_mig;
            int left = ns, np = 0;
            while ((left > 0 || !mig_done) && np < VGX_SOLO_MAX_PASS) {
                int pick[2] = {-1, -1}, n = 0;
                for (int sg = 0; sg < ns && n < 2; sg++)
                    if (!done[(size_t)sg] && (e->h_seg_par[(size_t)sg] < 0 || done[(size_t)e->h_seg_par[(size_t)sg]])) pick[n++] = sg;
                if (n < 2 && !mig_done) { pick[n++] = -2; mig_done = true; }
                for (int k = 0; k < 2; k++)
                    if (pick[k] >= 0) { done[(size_t)pick[k]] = 1; left--; }
                e->h_so_pass[(size_t)((2 * with_mig + 0) * VGX_SOLO_MAX_PASS + np)] = pick[0];
                e->h_so_pass[(size_t)((2 * with_mig + 1) * VGX_SOLO_MAX_PASS + np)] = pick[1];
                np++;
            }
            (with_mig ? e->h_so_npass1 : e->h_so_npass0) = (left > 0 || !mig_done) ? -1 : np;   // -1: does not fit
        }
    }
    {   // segments of the single-trajectory kernel: for every group the distinct non-zero susceptibility values, in group order
        e->h_so_sn.clear(); e->h_so_sig.clear();
        for (int64_t sn = 0; sn < S; sn++) {
            const size_t first = e->h_so_sn.size();
            for (size_t cb = 0; cb < cb_b.size(); cb++) {
                const double sg = cb_sig[cb * (size_t)S + (size_t)sn];
                if (sg == 0.0) continue;
                bool seen = false;
                for (size_t k = first; k < e->h_so_sn.size() && !seen; k++) seen = memcmp(&e->h_so_sig[k], &sg, 8) == 0;
                if (!seen) { e->h_so_sn.push_back((int32_t)sn); e->h_so_sig.push_back(sg); }
            }
        }
    }
    {   // susceptibility classes of the single-trajectory kernel's compact layout: haplotypes with identical susceptibility rows
        std::unordered_map<std::string, int> cmap;
        e->h_so_hapcls.assign((size_t)H, 0);
        e->h_so_nnz.assign(VGX_SOLO_ROWS, 0);
        e->h_so_tsn.assign(VGX_SOLO_ROWS * VGX_SOLO_MAX_S, 0);
        e->h_so_tsig.assign(VGX_SOLO_ROWS * VGX_SOLO_MAX_S, 0.0);
        e->h_so_clssig.assign(VGX_SOLO_ROWS * VGX_SOLO_MAX_S, 0.0);
        e->h_so_ncls = 0; e->h_so_maxnnz = 0;
        for (int64_t h = 0; h < H; h++) {
            std::string k((const char *)&p->susceptibility[h * S], (size_t)S * 8);
            auto it = cmap.find(k);
            int c;
            if (it == cmap.end()) {
                c = (int)cmap.size();
                cmap.emplace(k, c);
                if (c < VGX_SOLO_ROWS && S <= VGX_SOLO_MAX_S) {
                    int n = 0;
                    for (int64_t sn = 0; sn < S; sn++) {
                        const double sg = p->susceptibility[h * S + sn];
                        e->h_so_clssig[(size_t)(c * VGX_SOLO_MAX_S + sn)] = sg;
                        if (sg == 0.0) continue;
                        e->h_so_tsn[(size_t)(c * VGX_SOLO_MAX_S + n)] = (int32_t)sn;
                        e->h_so_tsig[(size_t)(c * VGX_SOLO_MAX_S + n)] = sg;
                        n++;
                    }
                    e->h_so_nnz[(size_t)c] = n;
                    e->h_so_maxnnz = std::max(e->h_so_maxnnz, n);
                }
            } else {
                c = it->second;
            }
            e->h_so_hapcls[(size_t)h] = c;
        }
        e->h_so_ncls = (int)cmap.size();
    }
    TauSetTables ts;
    tau_set_tables(e->d, p, t, ts);
    e->h_class_pos = ts.class_pos;

    e->suscepCumul = t.suscepCumul;
    e->mig = t.mig;
    e->actualSizes = t.actualSizes;
    e->sizes.assign(p->sizes, p->sizes + P);
    e->h_startLD.assign(p->startLD, p->startLD + P);
    e->h_endLD.assign(p->endLD, p->endLD + P);
    e->h_cdBefore.assign(p->contactDensityBeforeLockdown, p->contactDensityBeforeLockdown + P);
    e->h_cdAfter.assign(p->contactDensityAfterLockdown, p->contactDensityAfterLockdown + P);
    e->h_has_mig = false;
    for (int64_t i = 0; i < P; i++)
        for (int64_t j = 0; j < P; j++)
            if (i != j && p->migrationRates[i * P + j] != 0.0) e->h_has_mig = true;
    if (S > 64) return fail(e, VGX_ERR_ARG, "vgx_set_params: at most 64 susceptibility groups are supported");
    // uniform mutation model (every haplotype has the same mRate / hapMutType rows): table for the tau kernels
    e->h_mut_uniform = ts.mut_uniform;
    memcpy(e->h_mutp, ts.mutp, sizeof(e->h_mutp));
    e->h_mut_total = 0.0;
    for (int64_t s2 = 0; s2 < sites && s2 < 16; s2++)
        for (int i = 0; i < 3; i++) e->h_mut_total += e->h_mutp[s2][i];
    const double maxEffectiveBirth = t.maxEffectiveBirth;

    int rc = 0;
    rc |= upload(e, e->p_cls, e->cls.data(), (size_t)H);
    rc |= upload(e, e->p_suscType, p->suscType, (size_t)H);
    rc |= upload(e, e->p_mRate, p->mRate, (size_t)(H * sites));
    rc |= upload(e, e->p_hapMutType, p->hapMutType, (size_t)(H * sites * 3));
    rc |= upload(e, e->p_bRate, p->bRate, (size_t)H);
    rc |= upload(e, e->p_susc, p->susceptibility, (size_t)(H * S));
    rc |= upload(e, e->p_cd, c_d.data(), c_d.size());
    rc |= upload(e, e->p_cs, c_s.data(), c_s.size());
    rc |= upload(e, e->p_ctm, c_tm.data(), c_tm.size());
    rc |= upload(e, e->p_cbidx, c_bidx.data(), c_bidx.size());
    rc |= upload(e, e->p_cstype, c_stype.data(), c_stype.size());
    rc |= upload(e, e->p_cbb, cb_b.data(), cb_b.size());
    rc |= upload(e, e->p_cbsig, cb_sig.data(), cb_sig.size());
    {
        static const int32_t zero_i = 0;
        static const double zero_d = 0.0;
        const size_t ns = e->h_seg_par.size();
        rc |= upload(e, e->q_segpar, ns ? e->h_seg_par.data() : &zero_i, ns ? ns : 1);
        rc |= upload(e, e->q_segsn, ns ? e->h_seg_sn.data() : &zero_i, ns ? ns : 1);
        rc |= upload(e, e->q_segsig, ns ? e->h_seg_sig.data() : &zero_d, ns ? ns : 1);
        rc |= upload(e, e->q_cbseg, e->h_cb_seg.data(), e->h_cb_seg.size());
    }
    {
        static const int32_t zero_i = 0;
        static const double zero_d = 0.0;
        const size_t ns = e->h_so_sn.size();
        rc |= upload(e, e->so_sn, ns ? e->h_so_sn.data() : &zero_i, ns ? ns : 1);
        rc |= upload(e, e->so_sig, ns ? e->h_so_sig.data() : &zero_d, ns ? ns : 1);
        std::vector<double> rcp((size_t)P);
        for (int64_t pn = 0; pn < P; pn++) rcp[(size_t)pn] = 1.0 / e->actualSizes[(size_t)pn];
        rc |= upload(e, e->so_rcp, rcp.data(), rcp.size());
        rc |= upload(e, e->so_hapcls, e->h_so_hapcls.data(), e->h_so_hapcls.size());
        rc |= upload(e, e->so_nnz, e->h_so_nnz.data(), e->h_so_nnz.size());
        rc |= upload(e, e->so_tsn, e->h_so_tsn.data(), e->h_so_tsn.size());
        rc |= upload(e, e->so_tsig, e->h_so_tsig.data(), e->h_so_tsig.size());
        rc |= upload(e, e->so_clssig, e->h_so_clssig.data(), e->h_so_clssig.size());
        rc |= upload(e, e->so_pass, e->h_so_pass.data(), e->h_so_pass.size());
        if (rc == 0 && hipStreamSynchronize(e->stream) != hipSuccess) rc = VGX_ERR_HIP;   // rcp goes out of scope
    }
    rc |= upload(e, e->p_sizes, p->sizes, (size_t)P);
    rc |= upload(e, e->p_cdBefore, p->contactDensityBeforeLockdown, (size_t)P);
    rc |= upload(e, e->p_cdAfter, p->contactDensityAfterLockdown, (size_t)P);
    rc |= upload(e, e->p_startLD, p->startLD, (size_t)P);
    rc |= upload(e, e->p_endLD, p->endLD, (size_t)P);
    rc |= upload(e, e->p_sampMult, p->samplingMultiplier, (size_t)P);
    rc |= upload(e, e->p_actualSizes, e->actualSizes.data(), (size_t)P);
    rc |= upload(e, e->p_mig, e->mig.data(), (size_t)(P * P));
    // uniform migration: one common off-diagonal probability and (hence) one common recomputed diagonal
    e->h_mig_uniform = e->h_has_mig && P >= 2 && P <= 1024;
    for (int64_t i = 0; i < P && e->h_mig_uniform; i++)
        for (int64_t j = 0; j < P; j++) {
            const double v = e->mig[(size_t)(i * P + j)];
            if (v != (i == j ? e->mig[0] : e->mig[1])) { e->h_mig_uniform = false; break; }
        }
    if (e->h_mig_uniform) { e->h_mig_d = e->mig[0]; e->h_mig_b = e->mig[1]; }
    rc |= upload(e, e->p_suscTrans, p->suscepTransition, (size_t)(S * S));
    rc |= upload(e, e->p_suscCumul, e->suscepCumul.data(), (size_t)S);
    if (rc) return VGX_ERR_HIP;
    HIPCHECK(e, hipStreamSynchronize(e->stream));  // the sources are caller/stack memory

    VgxDevParams &d = e->dp;
    d.H = (int32_t)H; d.P = (int32_t)P; d.S = (int32_t)S; d.sites = (int32_t)sites; d.C = e->C; d.CB = e->CB;
    d.cls = (const int32_t *)e->p_cls.p; d.suscType = (const int64_t *)e->p_suscType.p;
    d.mRate = (const double *)e->p_mRate.p; d.hapMutType = (const double *)e->p_hapMutType.p;
    d.bRate = (const double *)e->p_bRate.p; d.susc = (const double *)e->p_susc.p;
    d.c_d = (const double *)e->p_cd.p; d.c_s = (const double *)e->p_cs.p; d.c_tm = (const double *)e->p_ctm.p;
    d.c_bidx = (const int32_t *)e->p_cbidx.p; d.c_stype = (const int32_t *)e->p_cstype.p;
    d.cb_b = (const double *)e->p_cbb.p;
    d.cb_sigma = (const double *)e->p_cbsig.p;
    d.sizes = (const int64_t *)e->p_sizes.p; d.cdBefore = (const double *)e->p_cdBefore.p;
    d.cdAfter = (const double *)e->p_cdAfter.p; d.startLD = (const double *)e->p_startLD.p;
    d.endLD = (const double *)e->p_endLD.p; d.sampMult = (const double *)e->p_sampMult.p;
    d.actualSizes = (const double *)e->p_actualSizes.p; d.mig = (const double *)e->p_mig.p;
    d.suscepTransition = (const double *)e->p_suscTrans.p; d.suscepCumul = (const double *)e->p_suscCumul.p;
    d.maxEffectiveBirth = maxEffectiveBirth;
    d.recombination = e->recombination; d.genome_length = e->genome_length;
    d.sitesPosition = (const int64_t *)e->p_sitesPos.p;
    e->have_params = true;
    e->n_sets = 1;
    e->tau_staged = false;
    e->dev_state_valid = false;  // class ids in the occupancy lists refer to the old parameter rows
    return VGX_OK;
}

// The blocks of the installed parameter sets with the engine's recombination settings (shared by all sets), to the device
static int upload_param_sets(vgx_engine *e) {
    for (VgxDevParams &d : e->h_psets) {
        d.recombination = e->recombination; d.genome_length = e->genome_length;
        d.sitesPosition = (const int64_t *)e->p_sitesPos.p;
    }
    int rc = ensure(e, e->ps_blocks, e->h_psets.size() * sizeof(VgxDevParams));
    if (rc) return rc;
    HIPCHECK(e, hipMemcpy(e->ps_blocks.p, e->h_psets.data(), e->h_psets.size() * sizeof(VgxDevParams), hipMemcpyHostToDevice));
    return VGX_OK;
}

extern "C" int vgx_set_param_sets(vgx_engine *e, int64_t n_sets, const vgx_params *sets, const int32_t *set_of) {
    if (!e) return VGX_ERR_ARG;
    if (!sets || !set_of || n_sets < 1) return fail(e, VGX_ERR_ARG, "vgx_set_param_sets: needs at least one set and the map from replicate to set");
    const int64_t H = e->d.hapNum, P = e->d.popNum, S = e->d.susNum, sites = e->d.sites, R = e->R;
    for (int64_t r = 0; r < R; r++)
        if (set_of[r] < 0 || set_of[r] >= n_sets)
            return fail(e, VGX_ERR_ARG, "vgx_set_param_sets: set_of[" + std::to_string(r) + "] = " + std::to_string(set_of[r]) +
                                            " is outside [0, " + std::to_string(n_sets) + ")");
    for (int64_t g = 0; g < n_sets; g++) {
        if (!sets[g].sizes) return fail(e, VGX_ERR_ARG, "vgx_set_param_sets: set " + std::to_string(g) + ": null parameter array");
        if (memcmp(sets[g].sizes, sets[0].sizes, (size_t)P * 8) != 0)
            return fail(e, VGX_ERR_ARG, "vgx_set_param_sets: set " + std::to_string(g) + ": sizes differ from set 0's (every set runs "
                                        "from the one start state of vgx_set_state)");
    }
    if (n_sets == 1) return vgx_set_params(e, &sets[0]);
    if (S > 64) return fail(e, VGX_ERR_ARG, "vgx_set_param_sets: at most 64 susceptibility groups are supported");

    // every set's tables on the host first: a refused set leaves the engine as it was
    std::vector<ParamTables> tabs((size_t)n_sets);
    int maxC = 0, maxCB = 0;
    for (int64_t g = 0; g < n_sets; g++) {
        const std::string who = "vgx_set_param_sets: set " + std::to_string(g);
        std::string msg;
        const int rc = build_param_tables(e->d, &sets[g], who, tabs[(size_t)g], msg);
        if (rc) return fail(e, rc, msg);
        const int C = (int)tabs[(size_t)g].c_d.size(), CB = (int)tabs[(size_t)g].cb_b.size();
        const size_t lds = vgxi_direct_lds_bytes((int)P, (int)S, C, CB);
        if (lds > 160 * 1024)
            return fail(e, VGX_ERR_ARG, who + ": the population/class tables need " + std::to_string(lds) +
                                            " bytes of LDS per wavefront (limit 163840): too many populations x rate classes");
        maxC = std::max(maxC, C); maxCB = std::max(maxCB, CB);
    }
    // what the engine holds per model (host copies, the shared sizes, the other kernels' tables) is set 0's
    const int rc0 = vgx_set_params(e, &sets[0]);
    if (rc0) return rc0;

    // all sets' arrays in one device allocation, 16-byte aligned; the blocks point into it
    std::vector<char> blob;
    auto put = [&blob](const void *src, size_t bytes) {
        const size_t off = (blob.size() + 15) & ~(size_t)15;
        blob.resize(off + bytes);
        if (bytes) memcpy(blob.data() + off, src, bytes);
        return off;
    };
    e->h_psets.assign((size_t)n_sets, VgxDevParams{});
    e->sets_startLD.resize((size_t)(n_sets * P));
    for (int64_t g = 0; g < n_sets; g++) {
        const vgx_params &p = sets[g];
        const ParamTables &t = tabs[(size_t)g];
        VgxDevParams &d = e->h_psets[(size_t)g];
        d.H = (int32_t)H; d.P = (int32_t)P; d.S = (int32_t)S; d.sites = (int32_t)sites;
        d.C = (int32_t)t.c_d.size(); d.CB = (int32_t)t.cb_b.size();
        d.maxEffectiveBirth = t.maxEffectiveBirth;
        // (offsets for now: the allocation's address is added below)
#define VGX_PUT(field, src, count) d.field = (decltype(d.field))put((src), (size_t)(count) * sizeof(*d.field))
        VGX_PUT(cls, t.cls.data(), H); VGX_PUT(suscType, p.suscType, H);
        VGX_PUT(mRate, p.mRate, H * sites); VGX_PUT(hapMutType, p.hapMutType, H * sites * 3);
        VGX_PUT(bRate, p.bRate, H); VGX_PUT(susc, p.susceptibility, H * S);
        VGX_PUT(c_d, t.c_d.data(), d.C); VGX_PUT(c_s, t.c_s.data(), d.C); VGX_PUT(c_tm, t.c_tm.data(), d.C);
        VGX_PUT(c_bidx, t.c_bidx.data(), d.C); VGX_PUT(c_stype, t.c_stype.data(), d.C);
        VGX_PUT(cb_b, t.cb_b.data(), d.CB); VGX_PUT(cb_sigma, t.cb_sig.data(), (int64_t)d.CB * S);
        VGX_PUT(sizes, p.sizes, P);
        VGX_PUT(cdBefore, p.contactDensityBeforeLockdown, P); VGX_PUT(cdAfter, p.contactDensityAfterLockdown, P);
        VGX_PUT(startLD, p.startLD, P); VGX_PUT(endLD, p.endLD, P); VGX_PUT(sampMult, p.samplingMultiplier, P);
        VGX_PUT(actualSizes, t.actualSizes.data(), P); VGX_PUT(mig, t.mig.data(), P * P);
        VGX_PUT(suscepTransition, p.suscepTransition, S * S); VGX_PUT(suscepCumul, t.suscepCumul.data(), S);
#undef VGX_PUT
        std::copy(p.startLD, p.startLD + P, e->sets_startLD.begin() + g * P);
    }
    int rc = ensure(e, e->ps_blob, blob.size());
    if (rc) return rc;
    HIPCHECK(e, hipMemcpy(e->ps_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
    const char *base = (const char *)e->ps_blob.p;
    for (VgxDevParams &d : e->h_psets) {
#define VGX_AT(field) d.field = (decltype(d.field))(base + (size_t)d.field)
        VGX_AT(cls); VGX_AT(suscType); VGX_AT(mRate); VGX_AT(hapMutType); VGX_AT(bRate); VGX_AT(susc);
        VGX_AT(c_d); VGX_AT(c_s); VGX_AT(c_tm); VGX_AT(c_bidx); VGX_AT(c_stype); VGX_AT(cb_b); VGX_AT(cb_sigma);
        VGX_AT(sizes); VGX_AT(cdBefore); VGX_AT(cdAfter); VGX_AT(startLD); VGX_AT(endLD); VGX_AT(sampMult);
        VGX_AT(actualSizes); VGX_AT(mig); VGX_AT(suscepTransition); VGX_AT(suscepCumul);
#undef VGX_AT
    }
    rc = upload_param_sets(e);
    if (rc) return rc;
    rc = ensure(e, e->ps_setof, (size_t)R * 4);
    if (rc) return rc;
    HIPCHECK(e, hipMemcpy(e->ps_setof.p, set_of, (size_t)R * 4, hipMemcpyHostToDevice));
    e->sets_C = maxC; e->sets_CB = maxCB;
    e->h_setof.assign(set_of, set_of + R);
    e->h_sets.assign((size_t)n_sets, TauSetTables{});
    for (int64_t g = 0; g < n_sets; g++) tau_set_tables(e->d, &sets[g], tabs[(size_t)g], e->h_sets[(size_t)g]);
    e->n_sets = n_sets;
    return VGX_OK;
}

extern "C" int vgx_set_recombination(vgx_engine *e, double recombination_probability, int64_t genome_length,
                                     const int64_t *sitesPosition) {
    if (!e) return VGX_ERR_ARG;
    const int64_t sites = e->d.sites;
    if (!(recombination_probability >= 0.0 && recombination_probability <= 1.0) || genome_length < 0)
        return fail(e, VGX_ERR_ARG, "vgx_set_recombination: probability outside [0, 1] or negative genome length");
    if (recombination_probability != 0.0 && (sites < 2 || !sitesPosition))
        return fail(e, VGX_ERR_ARG, "vgx_set_recombination: recombination needs at least two sites and their positions "
                                    "(the reference allocates its scratch vector only then, pyx:98-102)");
    HIPCHECK(e, hipSetDevice(e->device));
    e->recombination = recombination_probability;
    e->genome_length = genome_length;
    if (sites > 0 && sitesPosition) {
        int rc = upload(e, e->p_sitesPos, sitesPosition, (size_t)sites);
        if (rc) return rc;
        HIPCHECK(e, hipStreamSynchronize(e->stream));
    }
    e->dp.recombination = e->recombination; e->dp.genome_length = e->genome_length;
    e->dp.sitesPosition = (const int64_t *)e->p_sitesPos.p;
    if (e->n_sets > 1) return upload_param_sets(e);
    return VGX_OK;
}

extern "C" int vgx_get_recombinations(vgx_engine *e, int64_t replicate, int64_t cap, int64_t *idevents, int64_t *his,
                                      int64_t *hi2s, int64_t *nhis, int64_t *posRecombs, int64_t *n) {
    if (!e || !n || replicate < 0 || replicate >= e->R) return VGX_ERR_ARG;
    if (!e->sc_host_valid) return fail(e, VGX_ERR_ARG, "vgx_get_recombinations: no simulate call yet");
    *n = 0;
    if (e->last_was_tau || e->rec_cap == 0) return VGX_OK;   // (rec_cap is set by calls with recombination only)
    HIPCHECK(e, hipSetDevice(e->device));
    int64_t cnt = std::min<int64_t>(e->sc_host[(size_t)replicate].rec_n, e->rec_cap);
    *n = cnt;
    cnt = std::min(cnt, cap);
    if (cnt <= 0) return VGX_OK;
    std::vector<int64_t> rec((size_t)cnt * 5);
    HIPCHECK(e, hipMemcpy(rec.data(), (int64_t *)e->r_rec.p + replicate * e->rec_cap * 5, (size_t)cnt * 40, hipMemcpyDeviceToHost));
    int64_t *dst[5] = {idevents, his, hi2s, nhis, posRecombs};
    for (int c = 0; c < 5; c++)
        if (dst[c])
            for (int64_t i = 0; i < cnt; i++) dst[c][i] = rec[(size_t)(i * 5 + c)];
    return VGX_OK;
}

extern "C" int vgx_set_state(vgx_engine *e, const vgx_state *s) {
    if (!e || !s) return VGX_ERR_ARG;
    const int64_t H = e->d.hapNum, P = e->d.popNum, S = e->d.susNum;
    if (!s->susceptible || !s->infectious || !s->lockdownON || !s->contactDensity)
        return fail(e, VGX_ERR_ARG, "vgx_set_state: susceptible, infectious, lockdownON and contactDensity are required");
    HostState &h = e->hs;
    h.susceptible.assign(s->susceptible, s->susceptible + P * S);
    h.infectious.assign(s->infectious, s->infectious + P * H);
    if (s->initial_susceptible) h.initial_susceptible.assign(s->initial_susceptible, s->initial_susceptible + P * S);
    else h.initial_susceptible.assign((size_t)(P * S), 0);
    if (s->initial_infectious) h.initial_infectious.assign(s->initial_infectious, s->initial_infectious + P * H);
    else h.initial_infectious.assign((size_t)(P * H), 0);
    h.lockdownON.assign(s->lockdownON, s->lockdownON + P);
    h.contactDensity.assign(s->contactDensity, s->contactDensity + P);
    h.totalSusceptible.assign((size_t)P, 0);
    h.totalInfectious.assign((size_t)P, 0);
    if (s->totalSusceptible) h.totalSusceptible.assign(s->totalSusceptible, s->totalSusceptible + P);
    if (s->totalInfectious) h.totalInfectious.assign(s->totalInfectious, s->totalInfectious + P);
    h.first_simulation = s->first_simulation;
    h.globalInfectious = s->globalInfectious;
    h.bCounter = s->bCounter; h.dCounter = s->dCounter; h.sCounter = s->sCounter; h.mCounter = s->mCounter;
    h.iCounter = s->iCounter; h.swapLockdown = s->swapLockdown; h.migPlus = s->migPlus; h.migNonPlus = s->migNonPlus;
    h.good_attempt = s->good_attempt;
    h.currentTime = s->currentTime; h.totalRate = s->totalRate; h.totalMigrationRate = s->totalMigrationRate;
    h.tau_l = s->tau_l;
    h.ev_ptr = s->ev_ptr; h.ev_size = s->ev_size;
    e->have_state = true;
    e->dev_state_valid = false;
    e->tau_staged = false;
    return VGX_OK;
}

// ------------------------------------------------------------------------------------------------
// The host clock.  The reference advances currentTime with the C library's log() (SampleTime, pyx:476-478:
// currentTime += -log(u) / (totalRate + totalMigrationRate)), which is neither correctly rounded nor the same on every
// CPU; the device cannot reproduce it, and time never feeds back into the dynamics.  So the kernels log, per recorded
// event, the denominator of its time step and the index of its loop iteration, and the times are accumulated HERE, with
// this host's libm, from the same PCG64 stream (uniform 2j of the attempt's stream is iteration j's time draw,
// pyx:477,488): event times, the final currentTime and the lockdown timestamps come out as the reference computes them,
// bit for bit on a host whose libm matches.  Rejected migrations (pyx:691-692) leave the state and therefore the
// denominator unchanged, so every iteration between two records uses the later record's denominator.
struct ClockRun {      // accumulates one attempt's clock
    VgxPcg64 g;
    bool philox = false;   // the call drew from the counter-based stream: iteration i took outputs 2 i (time) and 2 i + 1 (event)
    uint64_t seed_ = 0;
    uint32_t att_ = 0;
    int64_t iter = 0;
    double t = 0.0;
    void open(int64_t seed, int64_t attempt, double t0) {
        vgx_pcg64_seed(g, (uint64_t)seed, (uint32_t)attempt);
        seed_ = (uint64_t)seed; att_ = (uint32_t)attempt;
        iter = 0; t = t0;
    }
    void advance(int64_t to_iter, double rate) {
        while (iter < to_iter) {
            double u;
            if (philox) {
                u = vgx_philox_stream_double(seed_, att_, 2 * (uint64_t)iter);
            } else {
                u = vgx_pcg64_double(g);
                (void)vgx_pcg64_next(g);             // the event's own uniform (pyx:488)
            }
            t += -std::log(u) / rate;
            iter++;
        }
    }
};

// The clock of replicate `rep` into `hc` (re-entrant: reads the engine only; a failure's message goes to `err`).
#define CLOCKCHECK(call)                                                                               \
    do {                                                                                               \
        hipError_t err__ = (call);                                                                     \
        if (err__ != hipSuccess) {                                                                     \
            err = std::string(#call) + ": " + hipGetErrorString(err__);                                \
            return VGX_ERR_HIP;                                                                        \
        }                                                                                              \
    } while (0)
// `staged`: the replicate's rate log and iteration indices already on the host (vgx_get_timelines packs them on the device and
// copies them to pinned memory); without it they are copied out of the device log here.
struct ClockStaged { const double *rate; const int32_t *iter; };
static int clock_build(const vgx_engine *e, int64_t rep, vgx_engine::HostClock &hc, std::string &err, const ClockStaged *staged = nullptr) {
    const VgxRepScalars &s = e->sc_host[(size_t)rep];
    hc.rep = -1;
    hc.times.clear();
    hc.loc_times.clear();
    hc.limit_mismatch = false;
    const bool rewound = s.restarts > 0;
    hc.e0 = rewound ? 0 : ((size_t)rep < e->call_ev0.size() ? e->call_ev0[(size_t)rep] : e->ev_ptr0);
    const int64_t n = std::max<int64_t>(s.ev_ptr - hc.e0, 0);
    const int64_t nloc = std::min<int64_t>(s.loc_n, e->loc_cap);
    std::vector<double> loc_dev((size_t)nloc);
    std::vector<int64_t> loc_key((size_t)nloc);
    if (nloc > 0) {
        CLOCKCHECK(hipMemcpy(loc_dev.data(), (double *)e->r_loctime.p + rep * e->loc_cap, (size_t)nloc * 8, hipMemcpyDeviceToHost));
        CLOCKCHECK(hipMemcpy(loc_key.data(), (int64_t *)e->r_lociter.p + rep * e->loc_cap, (size_t)nloc * 8, hipMemcpyDeviceToHost));
    }
    hc.loc_times = loc_dev;
    hc.final_time = s.currentTime;
    hc.exact = e->call_recorded;
    if (!e->call_recorded) {       // no rate log: the device clock (vgx_log) is all there is
        hc.rep = rep;
        return VGX_OK;
    }
    const double t_call = e->call_t0[(size_t)rep];
    const int64_t seed = e->seeds[(size_t)rep];
    const int64_t IT = ((int64_t)1 << 40) - 1;
    // lockdown records written outside the event loop (PrepareParameters / Restart): the attempt's start time
    for (int64_t i = 0; i < nloc; i++)
        if ((loc_key[(size_t)i] & IT) == 0) hc.loc_times[(size_t)i] = (loc_key[(size_t)i] >> 40) == 0 ? t_call : 0.0;
    // failed attempts that switched a lockdown inside their loop: their own (rate, iteration) pairs
    const int64_t nfa = std::min<int64_t>(s.fa_n, e->fa_cap);
    if (nfa > 0) {
        std::vector<double> fr((size_t)nfa);
        std::vector<int64_t> fk((size_t)nfa);
        CLOCKCHECK(hipMemcpy(fr.data(), (double *)e->r_farate.p + rep * e->fa_cap, (size_t)nfa * 8, hipMemcpyDeviceToHost));
        CLOCKCHECK(hipMemcpy(fk.data(), (int64_t *)e->r_fakey.p + rep * e->fa_cap, (size_t)nfa * 8, hipMemcpyDeviceToHost));
        int64_t k = 0;
        while (k < nfa) {
            const int64_t att = fk[(size_t)k] >> 40;
            ClockRun c;
            c.philox = e->call_philox;
            c.open(seed, att, att == 0 ? t_call : 0.0);
            for (; k < nfa && (fk[(size_t)k] >> 40) == att; k++) {
                c.advance(fk[(size_t)k] & IT, fr[(size_t)k]);
                for (int64_t i = 0; i < nloc; i++)
                    if (loc_key[(size_t)i] == fk[(size_t)k]) hc.loc_times[(size_t)i] = c.t;
            }
        }
    }
    // the attempt whose events are in the log
    if (s.last_attempt < 0) {                 // no attempt drew a number
        hc.final_time = t_call;
    } else if (s.restarts > s.last_attempt) { // the last attempt failed too: Restart left currentTime = 0 (pyx:717)
        hc.final_time = 0.0;
    } else {
        const int64_t slot0 = hc.e0 - e->ev_base;
        if (slot0 < 0 || slot0 + n > e->evcap) { err = "host_clock: event range outside the device log"; return VGX_ERR_ARG; }
        std::vector<double> rate;
        std::vector<int32_t> cols;
        const double *rate_p = staged ? staged->rate : nullptr;
        const int32_t *iter_p = staged ? staged->iter : nullptr;   // the iteration index of event k is iter_p[k * iter_stride]
        const int64_t iter_stride = staged ? 1 : VGX_EV_COLS;
        if (!staged) {
            rate.resize((size_t)n);
            cols.resize((size_t)n * VGX_EV_COLS);
            rate_p = rate.data();
            iter_p = cols.data() + 5;
        }
        if (n > 0 && !staged) {
            CLOCKCHECK(hipMemcpy(rate.data(), (double *)e->r_evrate.p + rep * e->evcap + slot0, (size_t)n * 8, hipMemcpyDeviceToHost));
            CLOCKCHECK(hipMemcpy(cols.data(), (int32_t *)e->r_evcols.p + (rep * e->evcap + slot0) * VGX_EV_COLS,
                                  (size_t)n * VGX_EV_COLS * 4, hipMemcpyDeviceToHost));
        }
        ClockRun c;
        c.philox = e->call_philox;
        c.open(seed, s.last_attempt, rewound ? 0.0 : t_call);
        hc.times.resize((size_t)n);
        int64_t li = 0;
        while (li < nloc && ((loc_key[(size_t)li] >> 40) != s.last_attempt || (loc_key[(size_t)li] & IT) == 0)) li++;
        bool limit_ok = true;
        int64_t it = 0;
        for (int64_t k = 0; k < n; k++) {
            // iteration index: 32 bits logged, strictly increasing
            const uint32_t lo = (uint32_t)iter_p[(size_t)(k * iter_stride)];
            it += (int64_t)(uint32_t)(lo - (uint32_t)it);
            if (e->call_has_tlimit && it > c.iter + 1) {   // loop condition of the iterations without a record (pyx:407)
                ClockRun probe = c;
                probe.advance(it - 1, rate_p[(size_t)k]);
                if (!(probe.t < e->call_tlimit)) limit_ok = false;
            }
            c.advance(it, rate_p[(size_t)k]);
            hc.times[(size_t)k] = c.t;
            if (e->call_has_tlimit && k + 1 < n && !(c.t < e->call_tlimit)) limit_ok = false;
            while (li < nloc && (loc_key[(size_t)li] >> 40) == s.last_attempt && (loc_key[(size_t)li] & IT) == it) {
                hc.loc_times[(size_t)li] = c.t;
                li++;
            }
        }
        c.advance(s.last_attempt_loops, s.totalRate + s.totalMig);   // trailing iterations without a record
        hc.final_time = c.t;
        // The kernel took its `currentTime < time` decisions (pyx:407) on the device clock (vgx_log, < 1 ulp from the host's
        // log).  If an event time lands within rounding of the limit the two clocks can disagree on one stop decision; the
        // run is then the device clock's run (a getter must not fail after the work is done): times stay the host clock's,
        // the mismatch is kept for vgx_clock_mismatches().
        if (e->call_has_tlimit && (!limit_ok || ((s.currentTime < e->call_tlimit) != (hc.final_time < e->call_tlimit)))) {
            hc.limit_mismatch = true;
        }
    }
    hc.rep = rep;
    return VGX_OK;
}
#undef CLOCKCHECK

// the clock of one replicate, cached in e->hc (the getters of one replicate call it one after another)
int host_clock(vgx_engine *e, int64_t rep) {
    vgx_engine::HostClock &hc = e->hc;
    if (hc.rep == rep) return VGX_OK;
    hc.rep = -1;
    std::string err;
    const int rc = clock_build(e, rep, hc, err);
    if (rc) return fail(e, rc, err);
    if (hc.limit_mismatch) e->clock_mismatches += 1;
    return VGX_OK;
}

extern "C" int vgx_get_counters(vgx_engine *e, int64_t replicate, vgx_counters *out) {
    if (!e || !out || replicate < 0 || replicate >= e->R) return VGX_ERR_ARG;
    if (!e->sc_host_valid) return fail(e, VGX_ERR_ARG, "vgx_get_counters: no simulate call yet");
    const VgxRepScalars &s = e->sc_host[(size_t)replicate];
    memset(out, 0, sizeof(*out));
    out->ev_ptr = s.ev_ptr;
    out->ev_first_new = s.restarts > 0 ? 0 : ((!e->last_was_tau && (size_t)replicate < e->call_ev0.size()) ? e->call_ev0[(size_t)replicate] : e->ev_ptr0);
    if (e->last_was_tau) out->reserved[0] = s.traj_next;  // tau: events drawn (sum of channel multiplicities)
    if (e->last_was_tau && (size_t)replicate < e->tau_sieve_skipped.size()) out->reserved[3] = e->tau_sieve_skipped[(size_t)replicate];
    out->loop_iterations = s.loop_iterations;
    out->restarts = s.restarts;
    out->lockdown_records = s.loc_n;
    out->error = s.error;
    out->multievent_rows = s.mev_rows;
    if (!e->last_was_tau) { out->reserved[1] = s.last_attempt; out->reserved[2] = s.last_attempt_loops; }
    else out->reserved[1] = -1;
    out->reserved[4] = s.sCounter;
    return VGX_OK;
}

extern "C" int vgx_get_counters_all(vgx_engine *e, int64_t *out /* [R][4]: ev_ptr, loop_iterations, restarts, tau events drawn */) {
    if (!e || !out) return VGX_ERR_ARG;
    if (!e->sc_host_valid) return fail(e, VGX_ERR_ARG, "vgx_get_counters_all: no simulate call yet");
    for (int64_t r = 0; r < e->R; r++) {
        const VgxRepScalars &s = e->sc_host[(size_t)r];
        out[r * 4 + 0] = s.ev_ptr;
        out[r * 4 + 1] = s.loop_iterations;
        out[r * 4 + 2] = s.restarts;
        out[r * 4 + 3] = e->last_was_tau ? s.traj_next : 0;
    }
    return VGX_OK;
}

extern "C" int vgx_get_events(vgx_engine *e, int64_t replicate, int64_t first, int64_t count, double *times,
                              int64_t *types, int64_t *haplotypes, int64_t *populations, int64_t *newHaplotypes,
                              int64_t *newPopulations) {
    if (!e || replicate < 0 || replicate >= e->R || first < 0 || count < 0) return VGX_ERR_ARG;
    if (count == 0) return VGX_OK;
    HIPCHECK(e, hipSetDevice(e->device));
    if (e->last_was_tau) {  // MULTITYPE records (pyx:2325): [start, end) of the step's multievent rows
        const auto &lg = e->tau_log[(size_t)replicate];
        int64_t i0 = first - e->tau_ev_ptr0[(size_t)replicate];
        if (i0 < 0 || i0 + count > (int64_t)lg.size()) return fail(e, VGX_ERR_ARG, "vgx_get_events: range outside the last tau call");
        for (int64_t i = 0; i < count; i++) {
            const auto &st = lg[(size_t)(i0 + i)];
            if (times) times[i] = st.time;
            if (types) types[i] = VGX_MULTITYPE;
            if (haplotypes) haplotypes[i] = st.m0;
            if (populations) populations[i] = st.m1;
            if (newHaplotypes) newHaplotypes[i] = 0;
            if (newPopulations) newPopulations[i] = 0;
        }
        return VGX_OK;
    }
    int64_t slot0 = first - e->ev_base;
    if (slot0 < 0 || slot0 + count > e->evcap) return fail(e, VGX_ERR_ARG, "vgx_get_events: range outside the device log of the last call");
    if (!e->call_recorded) return fail(e, VGX_ERR_ARG, "vgx_get_events: the last call did not record events");
    std::vector<int32_t> cols((size_t)count * VGX_EV_COLS);
    HIPCHECK(e, hipMemcpy(cols.data(), (int32_t *)e->r_evcols.p + (replicate * e->evcap + slot0) * VGX_EV_COLS,
                          (size_t)count * VGX_EV_COLS * 4, hipMemcpyDeviceToHost));
    if (times) {   // accumulated on the host with libm, as the reference does (host_clock)
        int rc = host_clock(e, replicate);
        if (rc) return rc;
        const int64_t i0 = first - e->hc.e0;
        if (i0 < 0 || i0 + count > (int64_t)e->hc.times.size())
            return fail(e, VGX_ERR_ARG, "vgx_get_events: times exist for the events of the last call only");
        memcpy(times, e->hc.times.data() + i0, (size_t)count * 8);
    }
    int64_t *dst[5] = {types, haplotypes, populations, newHaplotypes, newPopulations};
    for (int c = 0; c < 5; c++)
        if (dst[c])
            for (int64_t i = 0; i < count; i++) dst[c][i] = cols[(size_t)(i * VGX_EV_COLS + c)];
    return VGX_OK;
}

extern "C" int vgx_get_tau_tries(vgx_engine *e, int64_t replicate, int64_t first, int64_t count, int32_t *out) {
    if (!e || !out || replicate < 0 || replicate >= e->R || first < 0 || count < 0) return VGX_ERR_ARG;
    if (!e->last_was_tau || (size_t)replicate >= e->tau_log.size()) return fail(e, VGX_ERR_ARG, "vgx_get_tau_tries: the last call was not vgx_simulate_tau");
    const auto &lg = e->tau_log[(size_t)replicate];
    if (first + count > (int64_t)lg.size()) return fail(e, VGX_ERR_ARG, "vgx_get_tau_tries: the last call made fewer steps");
    for (int64_t i = 0; i < count; i++) out[i] = lg[(size_t)(first + i)].tries;
    return VGX_OK;
}

extern "C" int vgx_get_lockdowns(vgx_engine *e, int64_t replicate, int64_t cap, int64_t *states, int64_t *populations,
                                 double *times, int64_t *n) {
    if (!e || !n || replicate < 0 || replicate >= e->R) return VGX_ERR_ARG;
    if (!e->sc_host_valid) return fail(e, VGX_ERR_ARG, "vgx_get_lockdowns: no simulate call yet");
    HIPCHECK(e, hipSetDevice(e->device));
    if (e->last_was_tau) {
        const auto &tt = e->tau_loc_time[(size_t)replicate];
        *n = (int64_t)tt.size();
        for (int64_t i = 0; i < std::min<int64_t>(*n, cap); i++) {
            if (states) states[i] = e->tau_loc_state[(size_t)replicate][(size_t)i];
            if (populations) populations[i] = e->tau_loc_pop[(size_t)replicate][(size_t)i];
            if (times) times[i] = tt[(size_t)i];
        }
        return VGX_OK;
    }
    int64_t cnt = std::min<int64_t>(e->sc_host[(size_t)replicate].loc_n, e->loc_cap);
    *n = cnt;
    cnt = std::min(cnt, cap);
    if (cnt <= 0) return VGX_OK;
    std::vector<int32_t> rec((size_t)cnt * 2);
    HIPCHECK(e, hipMemcpy(rec.data(), (int32_t *)e->r_locrec.p + replicate * e->loc_cap * 2, (size_t)cnt * 8, hipMemcpyDeviceToHost));
    int rch = host_clock(e, replicate);
    if (rch) return rch;
    const std::vector<double> &tt = e->hc.loc_times;
    for (int64_t i = 0; i < cnt; i++) {
        if (states) states[i] = rec[(size_t)(i * 2)];
        if (populations) populations[i] = rec[(size_t)(i * 2 + 1)];
        if (times) times[i] = tt[(size_t)i];
    }
    return VGX_OK;
}

extern "C" int vgx_get_multievents(vgx_engine *e, int64_t replicate, int64_t cap, int64_t *num, double *times,
                                   int64_t *types, int64_t *haplotypes, int64_t *populations, int64_t *newHaplotypes,
                                   int64_t *newPopulations, int64_t *n) {
    if (!e || !n || replicate < 0 || replicate >= e->R) return VGX_ERR_ARG;
    *n = 0;
    if (!e->last_was_tau) return VGX_OK;
    HIPCHECK(e, hipSetDevice(e->device));
    const auto &lg = e->tau_log[(size_t)replicate];
    int64_t rows = (lg.empty() || e->tau_mev_cap <= 0) ? 0 : lg.back().m1;   // no rows when the call did not record them
    *n = rows;
    rows = std::min(rows, cap);
    if (rows <= 0) return VGX_OK;
    const int64_t mev_cap = e->tau_mev_cap;
    if (mev_cap <= 0) return VGX_OK;  // the call did not record multievents
    std::vector<int64_t> buf((size_t)rows * 6);
    HIPCHECK(e, hipMemcpy(buf.data(), (int64_t *)e->t_mev.p + replicate * mev_cap * 6, (size_t)rows * 48, hipMemcpyDeviceToHost));
    size_t st = 0;
    for (int64_t i = 0; i < rows; i++) {
        while (st + 1 < lg.size() && i >= lg[st].m1) st++;
        if (num) num[i] = buf[(size_t)(i * 6)];
        if (times) times[i] = lg[st].time;
        if (types) types[i] = buf[(size_t)(i * 6 + 1)];
        if (haplotypes) haplotypes[i] = buf[(size_t)(i * 6 + 2)];
        if (populations) populations[i] = buf[(size_t)(i * 6 + 3)];
        if (newHaplotypes) newHaplotypes[i] = buf[(size_t)(i * 6 + 4)];
        if (newPopulations) newPopulations[i] = buf[(size_t)(i * 6 + 5)];
    }
    return VGX_OK;
}

extern "C" int vgx_get_multievents_all(vgx_engine *e, int64_t cap, int64_t *offsets /* [R + 1] */, int64_t *rows /* [cap][6] */,
                                       int64_t *steps /* [cap] */) {
    if (!e || !offsets || cap < 0) return VGX_ERR_ARG;
    const int64_t R = e->R;
    for (int64_t r = 0; r <= R; r++) offsets[r] = 0;
    if (!e->last_was_tau || e->tau_mev_cap <= 0 || (int64_t)e->tau_log.size() < R) return VGX_OK;   // no rows recorded
    int64_t most = 0;
    for (int64_t r = 0; r < R; r++) {
        const auto &lg = e->tau_log[(size_t)r];
        const int64_t n = lg.empty() ? 0 : lg.back().m1;
        offsets[r + 1] = offsets[r] + n;
        most = std::max(most, n);
    }
    if (!rows) return VGX_OK;                                                                       // sizing call
    if (cap < offsets[R]) return fail(e, VGX_ERR_ARG, "vgx_get_multievents_all: room for fewer rows than the call recorded");
    if (most == 0) return VGX_OK;
    HIPCHECK(e, hipSetDevice(e->device));
    const int64_t mev_cap = e->tau_mev_cap;
    if (most > mev_cap) return fail(e, VGX_ERR_ARG, "vgx_get_multievents_all: a replicate logged more rows than its block holds");
    // the replicates' row blocks lie mev_cap rows apart on the device: strided copies of the widest block, a batch of replicates at a time
    const int64_t batch = std::max<int64_t>(1, std::min<int64_t>(R, ((int64_t)1 << 28) / (most * 48)));
    std::vector<int64_t> buf((size_t)(batch * most * 6));
    for (int64_t r0 = 0; r0 < R; r0 += batch) {
        const int64_t nr = std::min(batch, R - r0);
        HIPCHECK(e, hipMemcpy2D(buf.data(), (size_t)most * 48, (int64_t *)e->t_mev.p + r0 * mev_cap * 6, (size_t)mev_cap * 48, (size_t)most * 48,
                                (size_t)nr, hipMemcpyDeviceToHost));
        for (int64_t r = r0; r < r0 + nr; r++) {
            const int64_t n = offsets[r + 1] - offsets[r];
            if (n <= 0) continue;
            memcpy(rows + offsets[r] * 6, buf.data() + (r - r0) * most * 6, (size_t)n * 48);
            if (steps) {
                const auto &lg = e->tau_log[(size_t)r];
                size_t st = 0;
                for (int64_t i = 0; i < n; i++) {
                    while (st + 1 < lg.size() && i >= lg[st].m1) st++;
                    steps[offsets[r] + i] = (int64_t)st;
                }
            }
        }
    }
    return VGX_OK;
}

extern "C" int vgx_get_tau_states_all(vgx_engine *e, int64_t *infectious /* [R][P][H] */, int64_t *susceptible /* [R][P][S] */,
                                      int64_t *counters /* [R][8] */, double *times /* [R] */) {
    if (!e) return VGX_ERR_ARG;
    if (!e->last_was_tau || !e->sc_host_valid) return fail(e, VGX_ERR_ARG, "vgx_get_tau_states_all: the last call was not vgx_simulate_tau");
    HIPCHECK(e, hipSetDevice(e->device));
    const int64_t R = e->R, H = e->d.hapNum, P = e->d.popNum, S = e->d.susNum;
    if (susceptible) HIPCHECK(e, hipMemcpy(susceptible, e->t_S.p, (size_t)(R * P * S) * 8, hipMemcpyDeviceToHost));
    if (infectious) {
        const int64_t n = R * P * H, part = std::min<int64_t>(n, (int64_t)1 << 26);
        std::unique_ptr<int32_t[]> inf32(new int32_t[(size_t)part]);
        for (int64_t i0 = 0; i0 < n; i0 += part) {
            const int64_t k = std::min(part, n - i0);
            HIPCHECK(e, hipMemcpy(inf32.get(), (int32_t *)e->t_I.p + i0, (size_t)k * 4, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < k; i++) infectious[i0 + i] = inf32[(size_t)i];
        }
    }
    for (int64_t r = 0; r < R; r++) {
        const VgxRepScalars &s = e->sc_host[(size_t)r];
        if (counters) {
            int64_t *c = counters + r * 8;
            c[0] = s.bCounter; c[1] = s.dCounter; c[2] = s.sCounter; c[3] = s.mCounter; c[4] = s.iCounter; c[5] = s.migPlus;
            c[6] = s.globalInfectious; c[7] = s.ev_ptr;
        }
        if (times) times[r] = s.currentTime;
    }
    return VGX_OK;
}

extern "C" int vgx_get_trajectories(vgx_engine *e, double *out, int out_is_device) {
    if (!e || !out) return VGX_ERR_ARG;
    if (e->traj_points <= 0) return fail(e, VGX_ERR_ARG, "vgx_get_trajectories: the last call recorded none");
    HIPCHECK(e, hipSetDevice(e->device));
    size_t bytes = (size_t)(e->R * e->traj_points * e->d.popNum * 2) * 8;
    HIPCHECK(e, hipMemcpy(out, e->r_traj.p, bytes, out_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return VGX_OK;
}

extern "C" hipError_t vgxi_launch_traj_i32(const double *src, int32_t *dst, int64_t n, hipStream_t stream);
extern "C" int vgx_get_trajectories_int(vgx_engine *e, int32_t *out_device) {
    if (!e || !out_device) return VGX_ERR_ARG;
    if (e->traj_points <= 0) return fail(e, VGX_ERR_ARG, "vgx_get_trajectories_int: the last call recorded none");
    for (int64_t pn = 0; pn < e->d.popNum; pn++)
        if (e->sizes[(size_t)pn] >= ((int64_t)1 << 31)) return fail(e, VGX_ERR_ARG, "vgx_get_trajectories_int: population sizes of 2^31 or more");
    HIPCHECK(e, hipSetDevice(e->device));
    HIPCHECK(e, vgxi_launch_traj_i32((const double *)e->r_traj.p, out_device, e->R * e->traj_points * e->d.popNum * 2, e->stream));
    HIPCHECK(e, hipStreamSynchronize(e->stream));
    return VGX_OK;
}

extern "C" int64_t vgx_clock_mismatches(const vgx_engine *e) { return e ? e->clock_mismatches : 0; }

extern "C" int vgx_get_state(vgx_engine *e, int64_t replicate, vgx_state *out) {
    if (!e || !out || replicate < 0 || replicate >= e->R) return VGX_ERR_ARG;
    if (e->last_was_tau && e->sc_host_valid) {
        HIPCHECK(e, hipSetDevice(e->device));
        const int64_t H = e->d.hapNum, P = e->d.popNum, S = e->d.susNum;
        const VgxRepScalars &s = e->sc_host[(size_t)replicate];
        HostState &h = e->hs;
        if (out->susceptible) HIPCHECK(e, hipMemcpy(out->susceptible, (int64_t *)e->t_S.p + replicate * P * S, (size_t)(P * S) * 8, hipMemcpyDeviceToHost));
        if (out->infectious) {
            std::unique_ptr<int32_t[]> inf32(new int32_t[(size_t)(P * H)]);   // (not zero-filled: it is overwritten at once)
            HIPCHECK(e, hipMemcpy(inf32.get(), (int32_t *)e->t_I.p + replicate * P * H, (size_t)(P * H) * 4, hipMemcpyDeviceToHost));
            int64_t *dst = out->infectious;
            const int32_t *src = inf32.get();
            for_parts(P * H, [&](int64_t b0, int64_t en, unsigned) { for (int64_t i = b0; i < en; i++) dst[i] = src[i]; });
        }
        if (out->initial_susceptible) memcpy(out->initial_susceptible, h.initial_susceptible.data(), (size_t)(P * S) * 8);
        if (out->initial_infectious) memcpy(out->initial_infectious, h.initial_infectious.data(), (size_t)(P * H) * 8);
        std::vector<int64_t> tot((size_t)P);
        std::vector<double> cd((size_t)P);
        std::vector<int32_t> lk((size_t)P);
        HIPCHECK(e, hipMemcpy(tot.data(), (int64_t *)e->t_totInf.p + replicate * P, (size_t)P * 8, hipMemcpyDeviceToHost));
        HIPCHECK(e, hipMemcpy(cd.data(), (double *)e->t_cd.p + replicate * P, (size_t)P * 8, hipMemcpyDeviceToHost));
        HIPCHECK(e, hipMemcpy(lk.data(), (int32_t *)e->t_lock.p + replicate * P, (size_t)P * 4, hipMemcpyDeviceToHost));
        std::vector<int64_t> sus((size_t)(P * S));
        HIPCHECK(e, hipMemcpy(sus.data(), (int64_t *)e->t_S.p + replicate * P * S, (size_t)(P * S) * 8, hipMemcpyDeviceToHost));
        for (int64_t pn = 0; pn < P; pn++) {
            if (out->totalInfectious) out->totalInfectious[pn] = tot[(size_t)pn];
            if (out->totalSusceptible) {
                int64_t t = 0;
                for (int64_t sn = 0; sn < S; sn++) t += sus[(size_t)(pn * S + sn)];
                out->totalSusceptible[pn] = t;
            }
            if (out->lockdownON) out->lockdownON[pn] = lk[(size_t)pn];
            if (out->contactDensity) out->contactDensity[pn] = cd[(size_t)pn];
        }
        out->first_simulation = h.first_simulation;
        out->globalInfectious = s.globalInfectious;
        out->bCounter = s.bCounter; out->dCounter = s.dCounter; out->sCounter = s.sCounter; out->mCounter = s.mCounter;
        out->iCounter = s.iCounter; out->swapLockdown = s.swapLockdown; out->migPlus = s.migPlus;
        out->migNonPlus = s.migNonPlus; out->good_attempt = s.good_attempt;
        out->currentTime = s.currentTime; out->totalRate = s.totalRate; out->totalMigrationRate = s.totalMig;
        out->tau_l = s.tau_l;
        out->ev_ptr = s.ev_ptr; out->ev_size = e->last_ev_size;
        return VGX_OK;
    }
    if (!e->dev_state_valid || !e->sc_host_valid) return fail(e, VGX_ERR_ARG, "vgx_get_state: no device state");
    HIPCHECK(e, hipSetDevice(e->device));
    const int64_t H = e->d.hapNum, P = e->d.popNum, S = e->d.susNum, cap = e->cap;
    const VgxRepScalars &s = e->sc_host[(size_t)replicate];
    std::vector<int64_t> popI((size_t)(PI_COUNT * P));
    std::vector<double> popD((size_t)(PD_COUNT * P));
    HIPCHECK(e, hipMemcpy(popI.data(), (int64_t *)e->r_popI.p + replicate * PI_COUNT * P, popI.size() * 8, hipMemcpyDeviceToHost));
    HIPCHECK(e, hipMemcpy(popD.data(), (double *)e->r_popD.p + replicate * PD_COUNT * P, popD.size() * 8, hipMemcpyDeviceToHost));
    if (out->susceptible)
        HIPCHECK(e, hipMemcpy(out->susceptible, (int64_t *)e->r_sus.p + replicate * P * S, (size_t)(P * S) * 8, hipMemcpyDeviceToHost));
    if (out->infectious) {
        if (!e->counts64_valid) {
            HIPCHECK(e, vgxi_launch_counts64(e->dr.lcnt32, e->dr.lcnt, e->R * P * cap, e->stream));
            HIPCHECK(e, hipStreamSynchronize(e->stream));
            e->counts64_valid = true;
        }
        std::vector<int32_t> nocc((size_t)P);
        HIPCHECK(e, hipMemcpy(nocc.data(), (int32_t *)e->r_nocc.p + replicate * P, (size_t)P * 4, hipMemcpyDeviceToHost));
        memset(out->infectious, 0, (size_t)(P * H) * 8);
        std::vector<int32_t> hap;
        std::vector<int64_t> cnt;
        for (int64_t pn = 0; pn < P; pn++) {
            int64_t n = nocc[(size_t)pn];
            if (n <= 0) continue;
            hap.resize((size_t)n);
            cnt.resize((size_t)n);
            HIPCHECK(e, hipMemcpy(hap.data(), (int32_t *)e->r_lhap.p + (replicate * P + pn) * cap, (size_t)n * 4, hipMemcpyDeviceToHost));
            HIPCHECK(e, hipMemcpy(cnt.data(), (int64_t *)e->r_lcnt.p + (replicate * P + pn) * cap, (size_t)n * 8, hipMemcpyDeviceToHost));
            for (int64_t k = 0; k < n; k++) out->infectious[pn * H + hap[(size_t)k]] = cnt[(size_t)k];
        }
    }
    HostState &h = e->hs;
    if (out->initial_susceptible) memcpy(out->initial_susceptible, h.initial_susceptible.data(), (size_t)(P * S) * 8);
    if (out->initial_infectious) memcpy(out->initial_infectious, h.initial_infectious.data(), (size_t)(P * H) * 8);
    for (int64_t pn = 0; pn < P; pn++) {
        if (out->totalSusceptible) out->totalSusceptible[pn] = popI[(size_t)(PI_TOTSUS * P + pn)];
        if (out->totalInfectious) out->totalInfectious[pn] = popI[(size_t)(PI_TOTINF * P + pn)];
        if (out->lockdownON) out->lockdownON[pn] = popI[(size_t)(PI_LOCK * P + pn)];
        if (out->contactDensity) out->contactDensity[pn] = popD[(size_t)(PD_CD * P + pn)];
    }
    out->first_simulation = h.first_simulation;
    out->globalInfectious = s.globalInfectious;
    out->bCounter = s.bCounter; out->dCounter = s.dCounter; out->sCounter = s.sCounter; out->mCounter = s.mCounter;
    out->iCounter = s.iCounter; out->swapLockdown = s.swapLockdown; out->migPlus = s.migPlus;
    out->migNonPlus = s.migNonPlus; out->good_attempt = s.good_attempt;
    {
        int rch = host_clock(e, replicate);
        if (rch) return rch;
    }
    out->currentTime = e->hc.final_time; out->totalRate = s.totalRate; out->totalMigrationRate = s.totalMig;
    out->tau_l = s.tau_l;
    out->ev_ptr = s.ev_ptr; out->ev_size = e->last_ev_size;
    return VGX_OK;
}

extern "C" int vgx_get_list_counts_quad(vgx_engine *e, int64_t replicate, int64_t population, int64_t count, int32_t *out, int64_t *list_cap) {
    if (!e || replicate < 0 || replicate >= e->R || population < 0 || population >= e->d.popNum || count < 0) return VGX_ERR_ARG;
    if (list_cap) *list_cap = e->dev_state_valid ? e->cap : 0;
    if (count == 0) return VGX_OK;
    if (!out || !e->dev_state_valid || !e->counts32_valid || !e->dr.lcnt32 || count > e->cap) return VGX_ERR_ARG;
    HIPCHECK(e, hipSetDevice(e->device));
    HIPCHECK(e, hipMemcpy(out, e->dr.lcnt32 + (replicate * e->d.popNum + population) * e->cap, (size_t)count * 4, hipMemcpyDeviceToHost));
    return VGX_OK;
}

extern "C" int vgx_get_list_tile_sums(vgx_engine *e, int64_t replicate, int64_t population, int64_t count, int64_t *out, int64_t *tile_cap) {
    if (!e || replicate < 0 || replicate >= e->R || population < 0 || population >= e->d.popNum || count < 0) return VGX_ERR_ARG;
    if (tile_cap) *tile_cap = e->dev_state_valid ? e->dr.capT : 0;
    if (count == 0) return VGX_OK;
    if (!out || !e->dev_state_valid || !e->dr.ltsum || count > e->dr.capT) return VGX_ERR_ARG;
    HIPCHECK(e, hipSetDevice(e->device));
    HIPCHECK(e, hipStreamSynchronize(e->stream));
    HIPCHECK(e, hipMemcpy(out, e->dr.ltsum + (replicate * e->d.popNum + population) * e->dr.capT, (size_t)count * 8, hipMemcpyDeviceToHost));
    return VGX_OK;
}

extern "C" int vgx_get_profile(vgx_engine *e, int64_t replicate, int64_t *out16) {
    if (!e || !out16 || replicate < 0 || replicate >= e->R || !e->r_prof.p) return VGX_ERR_ARG;
    HIPCHECK(e, hipSetDevice(e->device));
    HIPCHECK(e, hipMemcpy(out16, (unsigned long long *)e->r_prof.p + replicate * VGX_PROF_SLOTS, VGX_PROF_SLOTS * 8, hipMemcpyDeviceToHost));
    return VGX_OK;
}

// ---- backward pass of many replicates on the device (vgx_genealogies.hip, vgx_gwalk.h) -------------------------------------
extern "C" int vgx_get_genealogies(vgx_engine *e, vgx_genealogies_io *io) {
    if (!e || !io || io->n < 0 || (io->n > 0 && (!io->replicates || !io->node_off || !io->mut_off || !io->mig_off)))
        return VGX_ERR_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    io->passes = 0;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    if (!e->sc_host_valid || !e->dev_state_valid) return fail(e, VGX_ERR_ARG, "vgx_get_genealogies: no direct simulate call yet");
    if (e->last_was_tau) return fail(e, VGX_ERR_ARG, "vgx_get_genealogies: the last call was vgx_simulate_tau (direct chains only)");
    if (!e->call_recorded) return fail(e, VGX_ERR_ARG, "vgx_get_genealogies: the last call did not record events");
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum;
    std::vector<int64_t> n_ev((size_t)n), sC((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const int64_t r = io->replicates[i];
        if (r < 0 || r >= e->R) return fail(e, VGX_ERR_ARG, "vgx_get_genealogies: replicate index out of range");
        const VgxRepScalars &s = e->sc_host[(size_t)r];
        const int64_t first = s.restarts > 0 ? 0 : ((size_t)r < e->call_ev0.size() ? e->call_ev0[(size_t)r] : e->ev_ptr0);
        if (first != 0 || e->ev_base != 0)
            return fail(e, VGX_ERR_ARG, "vgx_get_genealogies: the chain of replicate " + std::to_string(r) +
                                            " does not start in the last call's device log (events.ptr was not 0 at its start)");
        if (s.ev_ptr < 0 || s.ev_ptr > e->evcap || s.ev_ptr >= ((int64_t)1 << 30))
            return fail(e, VGX_ERR_ARG, "vgx_get_genealogies: event range of replicate " + std::to_string(r) + " outside the device log");
        n_ev[(size_t)i] = s.ev_ptr;
        sC[(size_t)i] = s.sCounter;
    }
    if (n == 0) return VGX_OK;
    HIPCHECK(e, hipSetDevice(e->device));
    const int32_t *log = (const int32_t *)e->r_evcols.p;

    if (!io->tree) {   // sizing: the log's MUTATION / MIGRATION events, counted on the device
        int64_t *d_rep = nullptr, *d_n = nullptr, *d_out = nullptr;
        std::vector<int64_t> cnt((size_t)n * 2);
        hipError_t er = hipMalloc(&d_rep, (size_t)n * 8 * 4);
        if (er != hipSuccess) return fail(e, VGX_ERR_HIP, std::string("vgx_get_genealogies: hipMalloc: ") + hipGetErrorString(er));
        d_n = d_rep + n;
        d_out = d_rep + 2 * n;
        er = hipMemcpy(d_rep, io->replicates, (size_t)n * 8, hipMemcpyHostToDevice);
        if (er == hipSuccess) er = hipMemcpy(d_n, n_ev.data(), (size_t)n * 8, hipMemcpyHostToDevice);
        if (er == hipSuccess) er = vgxi_gw_count(log, e->evcap, d_rep, d_n, n, d_out, e->stream);
        if (er == hipSuccess) er = hipStreamSynchronize(e->stream);
        if (er == hipSuccess) er = hipMemcpy(cnt.data(), d_out, (size_t)n * 16, hipMemcpyDeviceToHost);
        (void)hipFree(d_rep);
        if (er != hipSuccess) return fail(e, VGX_ERR_HIP, std::string("vgx_get_genealogies: counting pass: ") + hipGetErrorString(er));
        io->node_off[0] = io->mut_off[0] = io->mig_off[0] = 0;
        for (int64_t i = 0; i < n; i++) {
            const int64_t nodes = sC[(size_t)i] >= 2 ? 2 * sC[(size_t)i] - 1 : 0;
            io->node_off[i + 1] = io->node_off[i] + nodes;
            io->mut_off[i + 1] = io->mut_off[i] + cnt[(size_t)(2 * i)];
            io->mig_off[i + 1] = io->mig_off[i] + cnt[(size_t)(2 * i + 1)] + nodes;
        }
        io->ms[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
        return VGX_OK;
    }

    if (!io->rng_state || !io->tree_pop || !io->times || !io->status || !io->status_arg || !io->nodes_used || !io->mut_n || !io->mig_n ||
        !io->rng_out || (io->mut_off[n] > 0 && (!io->mut_node || !io->mut_AS || !io->mut_DS || !io->mut_site || !io->mut_time)) ||
        (io->mig_off[n] > 0 && (!io->mig_node || !io->mig_old || !io->mig_new || !io->mig_time)))
        return fail(e, VGX_ERR_ARG, "vgx_get_genealogies: null output");
    for (int64_t i = 0; i < n; i++) {
        const int64_t nodes = sC[(size_t)i] >= 2 ? 2 * sC[(size_t)i] - 1 : 0;
        if (io->node_off[i + 1] - io->node_off[i] < nodes || io->mut_off[i + 1] < io->mut_off[i] || io->mig_off[i + 1] < io->mig_off[i])
            return fail(e, VGX_ERR_ARG, "vgx_get_genealogies: output capacities smaller than the sizing call gave");
    }
    // the walk reads the 8-byte counts of the final occupancy lists
    if (!e->counts64_valid) {
        HIPCHECK(e, vgxi_launch_counts64(e->dr.lcnt32, e->dr.lcnt, e->R * P * e->cap, e->stream));
        HIPCHECK(e, hipStreamSynchronize(e->stream));
        e->counts64_valid = true;
    }
    // per-replicate workspace and outputs (elements), and the passes: every pass holds at most `share` bytes
    std::vector<VgxGwDesc> desc((size_t)n);
    std::vector<int64_t> bytes((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        VgxGwDesc &d = desc[(size_t)i];
        d.rep = io->replicates[i];
        d.n_ev = n_ev[(size_t)i];
        d.sCounter = sC[(size_t)i];
        d.tsize = d.sCounter >= 2 ? vgx_gw_table_size(d.n_ev, P * H) : 0;
        d.arena_cap = d.sCounter >= 2 ? d.n_ev : 0;
        d.mut_cap = io->mut_off[i + 1] - io->mut_off[i];
        d.mig_cap = io->mig_off[i + 1] - io->mig_off[i];
        for (int k = 0; k < 4; k++) d.rng[k] = io->rng_state[i * 4 + k];
        const int64_t nodes = d.sCounter >= 2 ? 2 * d.sCounter - 1 : 0;
        bytes[(size_t)i] = d.tsize * 28 + d.arena_cap * 4 + nodes * 12 + d.mut_cap * 20 + d.mig_cap * 16 + (int64_t)sizeof(VgxGwDesc) + 72;
    }
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    int64_t share = (int64_t)(free_b / 2);
    if (const char *cb = getenv("VGX_GENEALOGY_CHUNK_BYTES")) share = std::min<int64_t>(share, std::max<int64_t>(atoll(cb), 1));
    const bool wave = io->layout == 1;
    std::vector<int64_t> mism((size_t)n, 0);
    int64_t i0 = 0;
    while (i0 < n) {
        int64_t i1 = i0, sum = 0;
        while (i1 < n && (i1 == i0 || sum + bytes[(size_t)i1] <= share)) sum += bytes[(size_t)i1++];
        const int64_t m = i1 - i0;
        // offsets of this pass (element counts relative to the pass)
        int64_t T = 0, A = 0, N = 0, M = 0, G = 0;
        std::vector<VgxGwDesc> dp(desc.begin() + i0, desc.begin() + i1);
        for (int64_t j = 0; j < m; j++) {
            VgxGwDesc &d = dp[(size_t)j];
            d.tab_off = T; d.arena_off = A; d.node_off = N; d.mut_off = M; d.mig_off = G;
            T += d.tsize; A += d.arena_cap; N += d.sCounter >= 2 ? 2 * d.sCounter - 1 : 0; M += d.mut_cap; G += d.mig_cap;
        }
        // one allocation: [desc | res | rng | key | cnt | base | len | lcap | arena | node x3 | mut x5 | mig x4]
        auto up8 = [](int64_t b) { return (b + 255) / 256 * 256; };
        const int64_t o_desc = 0, o_res = o_desc + up8(m * (int64_t)sizeof(VgxGwDesc)), o_rng = o_res + up8(m * 40),
                      o_key = o_rng + up8(m * 32), o_cnt = o_key + up8(T * 8), o_base = o_cnt + up8(T * 8), o_len = o_base + up8(T * 4),
                      o_lcap = o_len + up8(T * 4), o_arena = o_lcap + up8(T * 4), o_out = o_arena + up8(A * 4),
                      out_bytes = up8((3 * N + 5 * M + 4 * G) * 4), total = o_out + out_bytes;
        char *ws = nullptr;
        hipError_t er = hipMalloc((void **)&ws, (size_t)total);
        if (er != hipSuccess)
            return fail(e, VGX_ERR_HIP, "vgx_get_genealogies: hipMalloc of " + std::to_string(total) + " bytes: " + hipGetErrorString(er));
        std::unique_ptr<char, void (*)(char *)> hold(ws, [](char *p) { (void)hipFree(p); });
        VgxGwLaunch a{};
        a.n = m;
        a.desc = (const VgxGwDesc *)(ws + o_desc);
        a.log = log; a.evcap = e->evcap;
        a.nocc = e->dr.nocc; a.lhap = e->dr.lhap; a.lcnt = e->dr.lcnt;
        a.P = P; a.H = H; a.cap = e->cap;
        a.key = (int64_t *)(ws + o_key); a.cnt = (int64_t *)(ws + o_cnt);
        a.base = (int32_t *)(ws + o_base); a.len = (int32_t *)(ws + o_len); a.lcap = (int32_t *)(ws + o_lcap);
        a.arena = (int32_t *)(ws + o_arena);
        int32_t *o32 = (int32_t *)(ws + o_out);
        a.tree = o32; a.tree_pop = o32 + N; a.node_ev = o32 + 2 * N;
        int32_t *mu = o32 + 3 * N;
        a.mut_node = mu; a.mut_AS = mu + M; a.mut_DS = mu + 2 * M; a.mut_site = mu + 3 * M; a.mut_ev = mu + 4 * M;
        int32_t *mg = mu + 5 * M;
        a.mig_node = mg; a.mig_old = mg + G; a.mig_new = mg + 2 * G; a.mig_ev = mg + 3 * G;
        a.res = (int64_t *)(ws + o_res);
        a.rng_out = (uint64_t *)(ws + o_rng);
        HIPCHECK(e, hipMemcpyAsync(ws + o_desc, dp.data(), (size_t)m * sizeof(VgxGwDesc), hipMemcpyHostToDevice, e->stream));
        if (T > 0) HIPCHECK(e, hipMemsetAsync(a.key, 0xFF, (size_t)T * 8, e->stream));   // every slot empty (-1)
        HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
        HIPCHECK(e, vgxi_gw_walk(&a, wave ? 1 : 0, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)
            return fail(e, VGX_ERR_HIP, std::string("vgx_get_genealogies: walk kernel failed: ") + hipGetErrorString(er));
        float kms = 0.f;
        HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
        io->ms[0] += kms;
        std::vector<int64_t> res((size_t)m * 5);
        std::vector<uint64_t> rng((size_t)m * 4);
        std::vector<int32_t> out((size_t)(3 * N + 5 * M + 4 * G));
        HIPCHECK(e, hipMemcpy(res.data(), a.res, (size_t)m * 40, hipMemcpyDeviceToHost));
        HIPCHECK(e, hipMemcpy(rng.data(), a.rng_out, (size_t)m * 32, hipMemcpyDeviceToHost));
        if (!out.empty()) HIPCHECK(e, hipMemcpy(out.data(), o32, out.size() * 4, hipMemcpyDeviceToHost));
        hold.reset();
        // event indices -> times through every replicate's host clock (re-entrant form, one replicate per thread at a time)
        const auto t_clock = std::chrono::steady_clock::now();
        const int32_t *h_tree = out.data(), *h_pop = h_tree + N, *h_nev = h_tree + 2 * N, *h_mu = h_tree + 3 * N, *h_mg = h_mu + 5 * M;
        std::vector<std::string> errs((size_t)m);
        std::vector<int> rcs((size_t)m, 0);
        int64_t work = 0;
        for (int64_t j = 0; j < m; j++) work += dp[(size_t)j].n_ev;
        for_parts(m, [&](int64_t j0, int64_t j1, unsigned) {
            if (hipSetDevice(e->device) != hipSuccess) { for (int64_t j = j0; j < j1; j++) { rcs[(size_t)j] = VGX_ERR_HIP; errs[(size_t)j] = "hipSetDevice"; } return; }
            vgx_engine::HostClock hc;
            for (int64_t j = j0; j < j1; j++) {
                const VgxGwDesc &d = dp[(size_t)j];
                const int64_t gi = i0 + j;
                int rc = clock_build(e, d.rep, hc, errs[(size_t)j]);
                if (rc) { rcs[(size_t)j] = rc; continue; }
                mism[(size_t)gi] = hc.limit_mismatch ? 1 : 0;
                const int64_t *r5 = res.data() + j * 5;
                io->status[gi] = r5[0]; io->status_arg[gi] = r5[1]; io->nodes_used[gi] = r5[2];
                io->mut_n[gi] = r5[0] == VGX_GW_OK ? r5[3] : 0;
                io->mig_n[gi] = r5[0] == VGX_GW_OK ? r5[4] : 0;
                for (int k = 0; k < 4; k++) io->rng_out[gi * 4 + k] = rng[(size_t)(j * 4 + k)];
                if (r5[0] != VGX_GW_OK) continue;
                auto time_of = [&](int32_t ev, double &t) {
                    if (ev < 0) { t = 0.0; return true; }
                    const int64_t k = (int64_t)ev - hc.e0;
                    if (k < 0 || k >= (int64_t)hc.times.size()) return false;
                    t = hc.times[(size_t)k];
                    return true;
                };
                bool ok = true;
                const int64_t nodes = 2 * d.sCounter - 1, no = io->node_off[gi];
                for (int64_t k = 0; k < nodes; k++) {
                    io->tree[no + k] = h_tree[d.node_off + k];
                    io->tree_pop[no + k] = h_pop[d.node_off + k];
                    ok &= time_of(h_nev[d.node_off + k], io->times[no + k]);
                }
                const int64_t mo = io->mut_off[gi];
                for (int64_t k = 0; k < r5[3]; k++) {
                    const int64_t q = d.mut_off + k;
                    io->mut_node[mo + k] = h_mu[q]; io->mut_AS[mo + k] = h_mu[M + q]; io->mut_DS[mo + k] = h_mu[2 * M + q];
                    io->mut_site[mo + k] = h_mu[3 * M + q];
                    ok &= time_of(h_mu[4 * M + q], io->mut_time[mo + k]);
                }
                const int64_t go = io->mig_off[gi];
                for (int64_t k = 0; k < r5[4]; k++) {
                    const int64_t q = d.mig_off + k;
                    io->mig_node[go + k] = h_mg[q]; io->mig_old[go + k] = h_mg[G + q]; io->mig_new[go + k] = h_mg[2 * G + q];
                    ok &= time_of(h_mg[3 * G + q], io->mig_time[go + k]);
                }
                if (!ok) { rcs[(size_t)j] = VGX_ERR_ARG; errs[(size_t)j] = "vgx_get_genealogies: an event index outside the host clock's range"; }
            }
        }, std::max<int64_t>(work / std::max<int64_t>(m, 1), 1) * 64);
        for (int64_t j = 0; j < m; j++)
            if (rcs[(size_t)j]) return fail(e, rcs[(size_t)j], errs[(size_t)j]);
        io->ms[1] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_clock).count();
        io->passes += 1;
        i0 = i1;
    }
    // every replicate's clock was built once, as when the replicates are fetched one by one
    for (int64_t i = 0; i < n; i++) e->clock_mismatches += mism[(size_t)i];
    io->ms[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    return VGX_OK;
}

// ---- log replays of many replicates on the device (vgx_timelines.hip, vgx_tline.h) ------------------------------------------
// The split of vgx_get_genealogies: the host runs every replicate's clock, here from the packed (iteration, rate)
// logs in pinned memory, and turns the times into step_num event indices per replicate; the device does the rest over the log
// in place.
extern "C" int vgx_get_timelines(vgx_engine *e, vgx_timelines_io *io) {
    if (!e || !io || io->n < 0 || (io->n > 0 && !io->replicates) || io->n_inf < 0 || io->n_sus < 0) return VGX_ERR_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    io->passes = 0;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    if (!e->sc_host_valid || !e->dev_state_valid) return fail(e, VGX_ERR_ARG, "vgx_get_timelines: needs a direct vgx_simulate_direct call with the event log first");
    if (e->last_was_tau) return fail(e, VGX_ERR_ARG, "vgx_get_timelines: the last call was vgx_simulate_tau (replays direct chains only)");
    if (!e->call_recorded) return fail(e, VGX_ERR_ARG, "vgx_get_timelines: the last call did not record events");
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, S = e->d.susNum, step = io->step_num, T = step + 1;
    const int64_t n_inf = io->n_inf, n_sus = io->n_sus;
    if (step < 1) return fail(e, VGX_ERR_ARG, "vgx_get_timelines: step_num must be at least 1");
    if (io->semantics != VGX_TL_REFERENCE && io->semantics != VGX_TL_COMPARTMENT)
        return fail(e, VGX_ERR_ARG, "vgx_get_timelines: semantics must be 0 (reference) or 1 (compartment)");
    if ((n_inf > 0 && (!io->inf_pop || !io->inf_hap)) || (n_sus > 0 && (!io->sus_pop || !io->sus_grp)) || n_inf + n_sus >= ((int64_t)1 << 20))
        return fail(e, VGX_ERR_ARG, "vgx_get_timelines: bad query list");
    {
        std::vector<std::pair<int64_t, int64_t>> qi, qs;
        for (int64_t k = 0; k < n_inf; k++) {
            if (io->inf_pop[k] < 0 || io->inf_pop[k] >= P) return fail(e, VGX_ERR_ARG, "vgx_get_timelines: population index out of range");
            if (io->inf_hap[k] < 0 || io->inf_hap[k] >= H) return fail(e, VGX_ERR_ARG, "vgx_get_timelines: haplotype index out of range");
            qi.emplace_back(io->inf_pop[k], io->inf_hap[k]);
        }
        for (int64_t k = 0; k < n_sus; k++) {
            if (io->sus_pop[k] < 0 || io->sus_pop[k] >= P) return fail(e, VGX_ERR_ARG, "vgx_get_timelines: population index out of range");
            if (io->sus_grp[k] < 0 || io->sus_grp[k] >= S) return fail(e, VGX_ERR_ARG, "vgx_get_timelines: susceptibility group index out of range");
            qs.emplace_back(io->sus_pop[k], io->sus_grp[k]);
        }
        std::sort(qi.begin(), qi.end());
        std::sort(qs.begin(), qs.end());
        if (std::adjacent_find(qi.begin(), qi.end()) != qi.end() || std::adjacent_find(qs.begin(), qs.end()) != qs.end())
            return fail(e, VGX_ERR_ARG, "vgx_get_timelines: a query is given twice");
    }
    std::vector<int32_t> n_ev((size_t)n);
    int64_t loc_need = 1;
    {
        std::vector<char> seen((size_t)e->R, 0);
        for (int64_t i = 0; i < n; i++) {
            const int64_t r = io->replicates[i];
            if (r < 0 || r >= e->R) return fail(e, VGX_ERR_ARG, "vgx_get_timelines: replicate index out of range");
            if (seen[(size_t)r]) return fail(e, VGX_ERR_ARG, "vgx_get_timelines: replicates must be distinct");
            seen[(size_t)r] = 1;
            const VgxRepScalars &s = e->sc_host[(size_t)r];
            const int64_t first = s.restarts > 0 ? 0 : ((size_t)r < e->call_ev0.size() ? e->call_ev0[(size_t)r] : e->ev_ptr0);
            if (first != 0 || e->ev_base != 0)
                return fail(e, VGX_ERR_ARG, "vgx_get_timelines: replicate " + std::to_string(r) + ": its chain does not start in the last call's device log (the model held " +
                                                std::to_string(e->ev_base != 0 ? e->ev_base : first) + " events when the ensemble started)");
            if (s.ev_ptr < 0 || s.ev_ptr > e->evcap || s.ev_ptr >= ((int64_t)1 << 30))
                return fail(e, VGX_ERR_ARG, "vgx_get_timelines: event range of replicate " + std::to_string(r) + " outside the device log");
            n_ev[(size_t)i] = (int32_t)s.ev_ptr;
            loc_need = std::max(loc_need, std::min<int64_t>(s.loc_n, e->loc_cap));
        }
    }
    if (!io->time_points) {   // sizing
        io->loc_cap = loc_need;
        io->ms[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
        return VGX_OK;
    }
    if (n == 0) {
        io->ms[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
        return VGX_OK;
    }
    if (!io->last_point || !io->loc_n || !io->loc_state || !io->loc_pop || !io->loc_time || (n_inf > 0 && (!io->inf_data || !io->inf_sample)) ||
        (n_sus > 0 && !io->sus_data))
        return fail(e, VGX_ERR_ARG, "vgx_get_timelines: null output");
    if (io->loc_cap < loc_need) return fail(e, VGX_ERR_ARG, "vgx_get_timelines: loc_cap smaller than the sizing call gave");
    const int64_t loc_cap = io->loc_cap;

    // the queries of every launch: as many as the LDS budget holds, infectious ones first
    int64_t budget = VGX_TL_LDS_DEFAULT;
    if (const char *lb = getenv("VGX_TIMELINES_LDS_BYTES")) budget = std::min<int64_t>(std::max<int64_t>(atoll(lb), 1), VGX_TL_LDS_MAX);
    const int64_t need1 = std::max(n_inf > 0 ? vgx_tl_lds_bytes(step, 1, 0) : 0, n_sus > 0 ? vgx_tl_lds_bytes(step, 0, 1) : vgx_tl_lds_bytes(step, 0, 0));
    if (need1 > VGX_TL_LDS_MAX)
        return fail(e, VGX_ERR_ARG, "vgx_get_timelines: step_num " + std::to_string(step) + " is too large: the counters of one query exceed a workgroup's LDS");
    budget = std::max(budget, need1);
    struct Group { int64_t i0, ni, s0, ns, tab_off, start_off; };
    std::vector<Group> groups;
    std::vector<int32_t> h_tab;
    std::vector<int64_t> h_start;
    for (int64_t i = 0, s = 0; i < n_inf || s < n_sus;) {
        Group g{i, 0, s, 0, (int64_t)h_tab.size(), (int64_t)h_start.size()};
        while (i + g.ni < n_inf && vgx_tl_lds_bytes(step, g.ni + 1, g.ns) <= budget) g.ni++;
        while (s + g.ns < n_sus && vgx_tl_lds_bytes(step, g.ni, g.ns + 1) <= budget) g.ns++;
        const int ts = vgx_tl_table_size((int)(g.ni + g.ns));
        h_tab.resize(h_tab.size() + (size_t)(3 * ts), -1);
        int32_t *tab = h_tab.data() + g.tab_off;
        for (int64_t k = 0; k < g.ni; k++) {
            vgx_tl_insert(tab, ts, 0, (int32_t)io->inf_pop[i + k], (int32_t)io->inf_hap[i + k], (int32_t)k);
            h_start.push_back(e->hs.initial_infectious[(size_t)(io->inf_pop[i + k] * H + io->inf_hap[i + k])]);
        }
        for (int64_t k = 0; k < g.ns; k++) {
            vgx_tl_insert(tab, ts, 1, (int32_t)io->sus_pop[s + k], (int32_t)io->sus_grp[s + k], (int32_t)(2 * g.ni + k));
            h_start.push_back(e->hs.initial_susceptible[(size_t)(io->sus_pop[s + k] * S + io->sus_grp[s + k])]);
        }
        groups.push_back(g);
        i += g.ni;
        s += g.ns;
    }
    HIPCHECK(e, hipSetDevice(e->device));
    auto up8 = [](int64_t b) { return (b + 255) / 256 * 256; };
    auto dev_free = [](char *p) { (void)hipFree(p); };
    char *qws = nullptr;
    const int64_t q_tab = 0, q_start = up8((int64_t)h_tab.size() * 4 + 8), q_total = q_start + up8((int64_t)h_start.size() * 8 + 8);
    hipError_t er = hipMalloc((void **)&qws, (size_t)q_total);
    if (er != hipSuccess) return fail(e, VGX_ERR_HIP, std::string("vgx_get_timelines: hipMalloc: ") + hipGetErrorString(er));
    std::unique_ptr<char, void (*)(char *)> qhold(qws, dev_free);
    if (!h_tab.empty()) HIPCHECK(e, hipMemcpy(qws + q_tab, h_tab.data(), h_tab.size() * 4, hipMemcpyHostToDevice));
    if (!h_start.empty()) HIPCHECK(e, hipMemcpy(qws + q_start, h_start.data(), h_start.size() * 8, hipMemcpyHostToDevice));

    // chunks of replicates: packed logs, cuts and outputs of a chunk fit `share` bytes of device memory (and 12 bytes per event
    // of pinned host memory)
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    int64_t share = std::min<int64_t>((int64_t)(free_b / 2), (int64_t)1 << 30);
    if (const char *cb = getenv("VGX_TIMELINES_CHUNK_BYTES")) share = std::min<int64_t>(share, std::max<int64_t>(atoll(cb), 1));
    const int64_t out_row = (2 * n_inf + n_sus) * T * 8;
    std::vector<int64_t> mism((size_t)n, 0);
    int64_t i0 = 0;
    while (i0 < n) {
        int64_t i1 = i0, sum = 0, E = 0, max_n = 0;
        while (i1 < n && i1 - i0 < ((int64_t)1 << 20)) {
            const int64_t b = (int64_t)n_ev[(size_t)i1] * 12 + step * 4 + out_row + 64;
            if (i1 > i0 && sum + b > share) break;
            sum += b;
            E += n_ev[(size_t)i1];
            max_n = std::max<int64_t>(max_n, n_ev[(size_t)i1]);
            i1++;
        }
        const int64_t m = i1 - i0;
        std::vector<int64_t> off((size_t)m), reps(io->replicates + i0, io->replicates + i1);
        for (int64_t j = 0, o = 0; j < m; j++) { off[(size_t)j] = o; o += n_ev[(size_t)(i0 + j)]; }
        // one allocation: [rep | n_ev | last | off | cut | iter | rate | inf | smp | sus]
        const int64_t o_rep = 0, o_nev = o_rep + up8(m * 8), o_last = o_nev + up8(m * 4), o_off = o_last + up8(m * 4), o_cut = o_off + up8(m * 8),
                      o_iter = o_cut + up8(m * step * 4), o_rate = o_iter + up8(E * 4), o_inf = o_rate + up8(E * 8),
                      o_smp = o_inf + up8(m * n_inf * T * 8), o_sus = o_smp + up8(m * n_inf * T * 8), total = o_sus + up8(m * n_sus * T * 8);
        char *ws = nullptr;
        er = hipMalloc((void **)&ws, (size_t)total);
        if (er != hipSuccess)
            return fail(e, VGX_ERR_HIP, "vgx_get_timelines: hipMalloc of " + std::to_string(total) + " bytes: " + hipGetErrorString(er));
        std::unique_ptr<char, void (*)(char *)> hold(ws, dev_free);
        const int64_t pin_iter = 0, pin_rate = up8(E * 4), pin_need = pin_rate + up8(E * 8);
        if ((int64_t)e->pin_tl_bytes < pin_need) {
            if (e->pin_tl) (void)hipHostFree(e->pin_tl);
            e->pin_tl = nullptr; e->pin_tl_bytes = 0;
            HIPCHECK(e, hipHostMalloc(&e->pin_tl, (size_t)pin_need, hipHostMallocDefault));
            e->pin_tl_bytes = (size_t)pin_need;
        }
        const int32_t *h_iter = (const int32_t *)((char *)e->pin_tl + pin_iter);
        const double *h_rate = (const double *)((char *)e->pin_tl + pin_rate);
        HIPCHECK(e, hipMemcpyAsync(ws + o_rep, reps.data(), (size_t)m * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(ws + o_nev, n_ev.data() + i0, (size_t)m * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(ws + o_off, off.data(), (size_t)m * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
        HIPCHECK(e, vgxi_tl_pack((const int32_t *)e->r_evcols.p, (const double *)e->r_evrate.p, e->evcap, (const int64_t *)(ws + o_rep),
                                 (const int32_t *)(ws + o_nev), (const int64_t *)(ws + o_off), m, max_n, (int32_t *)(ws + o_iter),
                                 (double *)(ws + o_rate), e->stream));
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        if (E > 0) {
            HIPCHECK(e, hipMemcpyAsync(e->pin_tl, ws + o_iter, (size_t)E * 4, hipMemcpyDeviceToHost, e->stream));
            HIPCHECK(e, hipMemcpyAsync((char *)e->pin_tl + pin_rate, ws + o_rate, (size_t)E * 8, hipMemcpyDeviceToHost, e->stream));
        }
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)
            return fail(e, VGX_ERR_HIP, std::string("vgx_get_timelines: pack kernel failed: ") + hipGetErrorString(er));
        float kms = 0.f;
        HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
        io->ms[0] += kms;
        // host: every replicate's clock -> time_points, cuts, last_point, lockdown times (one replicate per thread at a time)
        const auto t_clock = std::chrono::steady_clock::now();
        std::vector<int32_t> cuts((size_t)(m * step)), last((size_t)m);
        std::vector<std::string> errs((size_t)m);
        std::vector<int> rcs((size_t)m, 0);
        for_parts(m, [&](int64_t j0, int64_t j1, unsigned) {
            if (hipSetDevice(e->device) != hipSuccess) { for (int64_t j = j0; j < j1; j++) { rcs[(size_t)j] = VGX_ERR_HIP; errs[(size_t)j] = "hipSetDevice"; } return; }
            vgx_engine::HostClock hc;
            std::vector<int32_t> rec;
            for (int64_t j = j0; j < j1; j++) {
                const int64_t gi = i0 + j, r = reps[(size_t)j], ne = n_ev[(size_t)gi];
                const ClockStaged st{h_rate + off[(size_t)j], h_iter + off[(size_t)j]};
                int rc = clock_build(e, r, hc, errs[(size_t)j], &st);
                if (rc) { rcs[(size_t)j] = rc; continue; }
                if ((int64_t)hc.times.size() != ne) {
                    rcs[(size_t)j] = VGX_ERR_ARG;
                    errs[(size_t)j] = "vgx_get_timelines: the host clock of replicate " + std::to_string(r) + " does not cover its chain";
                    continue;
                }
                mism[(size_t)gi] = hc.limit_mismatch ? 1 : 0;
                double *tp = io->time_points + gi * T;
                vgx_tl_time_points(hc.final_time, step, tp);
                VgxTlCutter ct{tp, step, cuts.data() + j * step};
                for (int64_t k = 0; k < ne; k++) ct.event(k, hc.times[(size_t)k]);
                const int64_t lp = ct.finish(ne);
                last[(size_t)j] = (int32_t)lp;
                io->last_point[gi] = lp;
                const int64_t nloc = std::min<int64_t>(std::min<int64_t>(e->sc_host[(size_t)r].loc_n, e->loc_cap), (int64_t)hc.loc_times.size());
                io->loc_n[gi] = nloc;
                if (nloc > 0) {
                    rec.resize((size_t)nloc * 2);
                    hipError_t he = hipMemcpy(rec.data(), (int32_t *)e->r_locrec.p + r * e->loc_cap * 2, (size_t)nloc * 8, hipMemcpyDeviceToHost);
                    if (he != hipSuccess) { rcs[(size_t)j] = VGX_ERR_HIP; errs[(size_t)j] = std::string("vgx_get_timelines: lockdown records: ") + hipGetErrorString(he); continue; }
                    for (int64_t k = 0; k < nloc; k++) {
                        io->loc_state[gi * loc_cap + k] = rec[(size_t)(2 * k)];
                        io->loc_pop[gi * loc_cap + k] = rec[(size_t)(2 * k + 1)];
                        io->loc_time[gi * loc_cap + k] = hc.loc_times[(size_t)k];
                    }
                }
            }
        }, std::max<int64_t>(E / std::max<int64_t>(m, 1), 1) * 64);
        for (int64_t j = 0; j < m; j++)
            if (rcs[(size_t)j]) return fail(e, rcs[(size_t)j], errs[(size_t)j]);
        io->ms[1] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_clock).count();
        // device: the replay, one launch per group of queries
        HIPCHECK(e, hipMemcpyAsync(ws + o_cut, cuts.data(), (size_t)(m * step) * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(ws + o_last, last.data(), (size_t)m * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
        for (const Group &g : groups) {
            VgxTlLaunch a{};
            a.m = m;
            a.log = (const int32_t *)e->r_evcols.p; a.evcap = e->evcap;
            a.rep = (const int64_t *)(ws + o_rep); a.n_ev = (const int32_t *)(ws + o_nev); a.last = (const int32_t *)(ws + o_last);
            a.cut = (const int32_t *)(ws + o_cut);
            a.step = (int)step; a.semantics = (int)io->semantics;
            a.ni = (int)g.ni; a.ns = (int)g.ns; a.i0 = (int)g.i0; a.s0 = (int)g.s0; a.n_inf = (int)n_inf; a.n_sus = (int)n_sus;
            a.tsize = vgx_tl_table_size((int)(g.ni + g.ns));
            a.tab = (const int32_t *)(qws + q_tab) + g.tab_off;
            a.start = (const int64_t *)(qws + q_start) + g.start_off;
            a.inf = (double *)(ws + o_inf); a.smp = (double *)(ws + o_smp); a.sus = (double *)(ws + o_sus);
            HIPCHECK(e, vgxi_tl_replay(&a, e->stream));
            io->passes += 1;
        }
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)
            return fail(e, VGX_ERR_HIP, std::string("vgx_get_timelines: replay kernel failed: ") + hipGetErrorString(er));
        HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
        io->ms[0] += kms;
        if (n_inf > 0) {
            HIPCHECK(e, hipMemcpy(io->inf_data + i0 * n_inf * T, ws + o_inf, (size_t)(m * n_inf * T) * 8, hipMemcpyDeviceToHost));
            HIPCHECK(e, hipMemcpy(io->inf_sample + i0 * n_inf * T, ws + o_smp, (size_t)(m * n_inf * T) * 8, hipMemcpyDeviceToHost));
        }
        if (n_sus > 0) HIPCHECK(e, hipMemcpy(io->sus_data + i0 * n_sus * T, ws + o_sus, (size_t)(m * n_sus * T) * 8, hipMemcpyDeviceToHost));
        i0 = i1;
    }
    // every replicate's clock was built once, as when the replicates are fetched one by one
    for (int64_t i = 0; i < n; i++) e->clock_mismatches += mism[(size_t)i];
    io->ms[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    return VGX_OK;
}

// ---- the host clock of many replicates, chunk by chunk: what vgx_get_incidence and vgx_get_prevalence share ---------------------
// reps / n_ev: the selected replicates and the events of their chains, d_rep / d_nev the same on the device.  A chunk is as many
// consecutive replicates as `share` bytes of device memory (at most 2^30, or VGX_TIMELINES_CHUNK_BYTES) hold at 12 bytes per event,
// staged through pinned host memory; the log itself is not copied.  on_chain(i, times) gets the event times of selected
// replicate i (from several threads, one replicate each at a time), then on_chunk(i0, i1, max_n) runs the device pass over the
// replicates [i0, i1) and returns its code.  ms[0] gains the pack kernel's time, ms[1] the host clock's.  Every replicate's clock
// is built once, as when the replicates are fetched one by one: vgx_clock_mismatches counts each once.  With `tile` > 0 a chunk's
// replicates each also hold tile_bytes per tile of the chunk's longest chain (the bases of vgx_get_milestones), counted in `share`.
template <class Chain, class Chunk>
static int clock_chunks(vgx_engine *e, const char *what, const std::vector<int64_t> &reps, const std::vector<int32_t> &n_ev, const int64_t *d_rep,
                        const int32_t *d_nev, int64_t share, double *ms, Chain on_chain, Chunk on_chunk, int64_t tile = 0, int64_t tile_bytes = 0) {
    const std::string pre = std::string(what) + ": ";
    const int64_t n = (int64_t)reps.size();
    auto up8 = [](int64_t b) { return (b + 255) / 256 * 256; };
    auto dev_free = [](char *p) { (void)hipFree(p); };
    share = std::min<int64_t>(share, (int64_t)1 << 30);
    if (const char *cb = getenv("VGX_TIMELINES_CHUNK_BYTES")) share = std::min<int64_t>(share, std::max<int64_t>(atoll(cb), 1));
    std::vector<int64_t> mism((size_t)n, 0);
    int64_t i0 = 0;
    while (i0 < n) {
        int64_t i1 = i0, sum = 0, E = 0, max_n = 0;
        while (i1 < n && i1 - i0 < ((int64_t)1 << 20)) {
            const int64_t b = (int64_t)n_ev[(size_t)i1] * 12 + 64;
            // (vgx_get_milestones: every replicate of the chunk also holds tile_bytes per tile of the chunk's longest chain)
            const int64_t tiles = tile > 0 ? std::max<int64_t>((std::max<int64_t>(max_n, n_ev[(size_t)i1]) + tile - 1) / tile, 1) : 0;
            if (i1 > i0 && sum + b + (i1 - i0 + 1) * tiles * tile_bytes > share) break;
            sum += b;
            E += n_ev[(size_t)i1];
            max_n = std::max<int64_t>(max_n, n_ev[(size_t)i1]);
            i1++;
        }
        const int64_t m = i1 - i0;
        std::vector<int64_t> off((size_t)m);
        for (int64_t j = 0, o = 0; j < m; j++) { off[(size_t)j] = o; o += n_ev[(size_t)(i0 + j)]; }
        const int64_t o_off = 0, o_iter = o_off + up8(m * 8), o_rate = o_iter + up8(E * 4), total = o_rate + up8(E * 8);
        char *ws = nullptr;
        hipError_t er = hipMalloc((void **)&ws, (size_t)total);
        if (er != hipSuccess) return fail(e, VGX_ERR_HIP, pre + "hipMalloc of " + std::to_string(total) + " bytes: " + hipGetErrorString(er));
        std::unique_ptr<char, void (*)(char *)> hold(ws, dev_free);
        const int64_t pin_rate = up8(E * 4), pin_need = pin_rate + up8(E * 8);
        if ((int64_t)e->pin_tl_bytes < pin_need) {
            if (e->pin_tl) (void)hipHostFree(e->pin_tl);
            e->pin_tl = nullptr; e->pin_tl_bytes = 0;
            HIPCHECK(e, hipHostMalloc(&e->pin_tl, (size_t)pin_need, hipHostMallocDefault));
            e->pin_tl_bytes = (size_t)pin_need;
        }
        const int32_t *h_iter = (const int32_t *)e->pin_tl;
        const double *h_rate = (const double *)((char *)e->pin_tl + pin_rate);
        HIPCHECK(e, hipMemcpyAsync(ws + o_off, off.data(), (size_t)m * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
        HIPCHECK(e, vgxi_tl_pack((const int32_t *)e->r_evcols.p, (const double *)e->r_evrate.p, e->evcap, d_rep + i0, d_nev + i0,
                                 (const int64_t *)(ws + o_off), m, max_n, (int32_t *)(ws + o_iter), (double *)(ws + o_rate), e->stream));
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        if (E > 0) {
            HIPCHECK(e, hipMemcpyAsync(e->pin_tl, ws + o_iter, (size_t)E * 4, hipMemcpyDeviceToHost, e->stream));
            HIPCHECK(e, hipMemcpyAsync((char *)e->pin_tl + pin_rate, ws + o_rate, (size_t)E * 8, hipMemcpyDeviceToHost, e->stream));
        }
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, pre + "pack kernel failed: " + hipGetErrorString(er));
        float kms = 0.f;
        HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
        ms[0] += kms;
        const auto t_clock = std::chrono::steady_clock::now();
        std::vector<std::string> errs((size_t)m);
        std::vector<int> rcs((size_t)m, 0);
        for_parts(m, [&](int64_t j0, int64_t j1, unsigned) {
            if (hipSetDevice(e->device) != hipSuccess) { for (int64_t j = j0; j < j1; j++) { rcs[(size_t)j] = VGX_ERR_HIP; errs[(size_t)j] = "hipSetDevice"; } return; }
            vgx_engine::HostClock hc;
            for (int64_t j = j0; j < j1; j++) {
                const int64_t gi = i0 + j, r = reps[(size_t)gi], ne = n_ev[(size_t)gi];
                const ClockStaged st{h_rate + off[(size_t)j], h_iter + off[(size_t)j]};
                int rc = clock_build(e, r, hc, errs[(size_t)j], &st);
                if (rc) { rcs[(size_t)j] = rc; continue; }
                if ((int64_t)hc.times.size() != ne) {
                    rcs[(size_t)j] = VGX_ERR_ARG;
                    errs[(size_t)j] = pre + "the host clock of replicate " + std::to_string(r) + " does not cover its chain";
                    continue;
                }
                mism[(size_t)gi] = hc.limit_mismatch ? 1 : 0;
                on_chain(gi, hc.times);
            }
        }, std::max<int64_t>(E / std::max<int64_t>(m, 1), 1) * 64);
        for (int64_t j = 0; j < m; j++)
            if (rcs[(size_t)j]) return fail(e, rcs[(size_t)j], errs[(size_t)j]);
        ms[1] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_clock).count();
        const int rc = on_chunk(i0, i1, max_n);
        if (rc) return rc;
        i0 = i1;
    }
    for (int64_t i = 0; i < n; i++) e->clock_mismatches += mism[(size_t)i];
    return VGX_OK;
}

// ---- event counts per time bin of many replicates on the device (vgx_incidence.hip, vgx_incidence.h) ----------
// The split of vgx_get_timelines: the host runs every replicate's clock from the packed (iteration, rate) logs in pinned memory,
// chunk of replicates by chunk, and turns the times into T + 1 event indices per replicate; the device counts over the log in
// place into one block for all selected replicates, which the column summary then reads where it lies.
extern "C" int vgx_get_incidence(vgx_engine *e, vgx_incidence_io *io) {
    if (!e || !io || io->n < 0 || (io->n > 0 && (!io->replicates || !io->outside))) return VGX_ERR_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    auto wall = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(); };
    io->passes = 0;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    if (e->last_was_tau) return fail(e, VGX_ERR_ARG, "vgx_get_incidence: the last call was vgx_simulate_tau (counts direct chains only)");
    if (!e->sc_host_valid || !e->dev_state_valid) return fail(e, VGX_ERR_ARG, "vgx_get_incidence: needs a direct vgx_simulate_direct call with the event log first");
    if (!e->call_recorded) return fail(e, VGX_ERR_ARG, "vgx_get_incidence: the last call did not record events");
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, T = io->T, cells = P * VGX_INC_CHANNELS;
    if (T < 1 || T >= VGX_INC_MAX_BINS || !io->edges) return fail(e, VGX_ERR_ARG, "vgx_get_incidence: T = " + std::to_string(T) + " bins: at least 1, below 2^24, with edges");
    for (int64_t k = 0; k <= T; k++) {
        if (!std::isfinite(io->edges[k])) return fail(e, VGX_ERR_ARG, "vgx_get_incidence: edges[" + std::to_string(k) + "] is not finite");
        if (k > 0 && !(io->edges[k - 1] < io->edges[k]))
            return fail(e, VGX_ERR_ARG, "vgx_get_incidence: edges must increase strictly (edges[" + std::to_string(k) + "])");
    }
    if (vgx_inc_lds_bytes(P) > VGX_INC_LDS_MAX)
        return fail(e, VGX_ERR_ARG, "vgx_get_incidence: " + std::to_string(P) + " populations need " + std::to_string(vgx_inc_lds_bytes(P)) +
                                        " bytes of counters, above the " + std::to_string((int64_t)VGX_INC_LDS_MAX) + " bytes of LDS a counting workgroup may use");
    std::vector<int32_t> n_ev((size_t)n);
    {
        std::vector<char> seen((size_t)e->R, 0);
        for (int64_t i = 0; i < n; i++) {
            const int64_t r = io->replicates[i];
            if (r < 0 || r >= e->R) return fail(e, VGX_ERR_ARG, "vgx_get_incidence: replicate index out of range");
            if (seen[(size_t)r]) return fail(e, VGX_ERR_ARG, "vgx_get_incidence: replicates must be distinct");
            seen[(size_t)r] = 1;
            const VgxRepScalars &s = e->sc_host[(size_t)r];
            const int64_t first = s.restarts > 0 ? 0 : ((size_t)r < e->call_ev0.size() ? e->call_ev0[(size_t)r] : e->ev_ptr0);
            if (first != 0 || e->ev_base != 0)
                return fail(e, VGX_ERR_ARG, "vgx_get_incidence: replicate " + std::to_string(r) + ": its chain does not start in the last call's device log (the model held " +
                                                std::to_string(e->ev_base != 0 ? e->ev_base : first) + " events when the ensemble started)");
            if (s.ev_ptr >= VGX_INC_MAX_EVENTS)
                return fail(e, VGX_ERR_ARG, "vgx_get_incidence: replicate " + std::to_string(r) + " holds a chain of " + std::to_string(s.ev_ptr) + " events (2^30 or more)");
            if (s.ev_ptr < 0 || s.ev_ptr > e->evcap)
                return fail(e, VGX_ERR_ARG, "vgx_get_incidence: event range of replicate " + std::to_string(r) + " outside the device log");
            n_ev[(size_t)i] = (int32_t)s.ev_ptr;
        }
    }
    if (n == 0) {
        io->ms[2] = wall();
        return VGX_OK;
    }
    int64_t tile = VGX_INC_TILE_DEFAULT;
    if (const char *tb = getenv("VGX_INCIDENCE_TILE_EVENTS")) tile = std::min<int64_t>(std::max<int64_t>(atoll(tb), 1), VGX_INC_MAX_EVENTS);
    HIPCHECK(e, hipSetDevice(e->device));
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    auto up8 = [](int64_t b) { return (b + 255) / 256 * 256; };
    auto dev_free = [](char *p) { (void)hipFree(p); };
    // what stays for the whole call: [rep | n_ev | cut | mask | counts]
    const int64_t mask_words = (H + 31) / 32;
    const int64_t block_bytes = n * T * cells * 4;
    const int64_t o_rep = 0, o_nev = o_rep + up8(n * 8), o_cut = o_nev + up8(n * 4), o_mask = o_cut + up8(n * (T + 1) * 4),
                  o_cnt = o_mask + up8(mask_words * 4), keep_total = o_cnt + up8(block_bytes);
    if (keep_total > (int64_t)(free_b / 2))
        return fail(e, VGX_ERR_ARG, "vgx_get_incidence: the block of " + std::to_string(n) + " x " + std::to_string(T) + " x " + std::to_string(P) + " x 7 counts and its cuts take " +
                                        std::to_string(keep_total) + " bytes, above half of the " + std::to_string((int64_t)free_b) +
                                        " bytes of free device memory: select fewer replicates per call");
    char *kws = nullptr;
    hipError_t er = hipMalloc((void **)&kws, (size_t)keep_total);
    if (er != hipSuccess) return fail(e, VGX_ERR_HIP, "vgx_get_incidence: hipMalloc of " + std::to_string(keep_total) + " bytes: " + hipGetErrorString(er));
    std::unique_ptr<char, void (*)(char *)> khold(kws, dev_free);
    std::vector<int64_t> reps_all(io->replicates, io->replicates + n);
    HIPCHECK(e, hipMemcpyAsync(kws + o_rep, reps_all.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_nev, n_ev.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    if (io->hap_mask) HIPCHECK(e, hipMemcpyAsync(kws + o_mask, io->hap_mask, (size_t)mask_words * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemsetAsync(kws + o_cnt, 0, (size_t)block_bytes, e->stream));   // zeroed once

    const int64_t share = (int64_t)(free_b / 2) - keep_total + 4096;
    std::vector<int32_t> cuts((size_t)(n * (T + 1)));
    const int rc_chunks = clock_chunks(e, "vgx_get_incidence", reps_all, n_ev, (const int64_t *)(kws + o_rep), (const int32_t *)(kws + o_nev), share, io->ms,
        // host: a replicate's event times -> its T + 1 cuts
        [&](int64_t gi, const std::vector<double> &times) {
            int32_t *cut = cuts.data() + gi * (T + 1);
            VgxIncCutter ct{io->edges, T, cut};
            for (size_t k = 0; k < times.size(); k++) ct.event((int64_t)k, times[k]);
            ct.finish((int64_t)times.size());
            io->outside[2 * gi] = cut[0];
            io->outside[2 * gi + 1] = (int64_t)times.size() - cut[(size_t)T];
        },
        // device: the count of the chunk's replicates into their rows of the block
        [&](int64_t i0, int64_t i1, int64_t max_n) -> int {
            const int64_t m = i1 - i0;
            HIPCHECK(e, hipMemcpyAsync(kws + o_cut + i0 * (T + 1) * 4, cuts.data() + i0 * (T + 1), (size_t)(m * (T + 1)) * 4, hipMemcpyHostToDevice, e->stream));
            HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
            VgxIncLaunch a{};
            a.m = m;
            a.log = (const int32_t *)e->r_evcols.p; a.evcap = e->evcap;
            a.rep = (const int64_t *)(kws + o_rep) + i0; a.n_ev = (const int32_t *)(kws + o_nev) + i0;
            a.cut = (const int32_t *)(kws + o_cut) + i0 * (T + 1);
            a.T = (int32_t)T; a.P = (int32_t)P; a.hapNum = (int32_t)H;
            a.mask = io->hap_mask ? (const uint32_t *)(kws + o_mask) : nullptr;
            a.tile = (int32_t)tile; a.max_n = max_n;
            a.counts = (int32_t *)(kws + o_cnt) + i0 * T * cells;
            HIPCHECK(e, vgxi_inc_count(&a, e->stream));
            if (max_n > 0) io->passes += 1;
            HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
            if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)
                return fail(e, VGX_ERR_HIP, std::string("vgx_get_incidence: counting kernel failed: ") + hipGetErrorString(er));
            float kms = 0.f;
            HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
            io->ms[0] += kms;
            return VGX_OK;
        });
    if (rc_chunks) return rc_chunks;
    if (io->summary) {
        char msg[512] = "";
        const int rc = vgxi_column_summary_i32("vgx_get_incidence: summary", (const int32_t *)(kws + o_cnt), n, T * cells, io->summary, e->stream, msg, sizeof msg);
        if (rc) return fail(e, rc, msg);
    }
    if (io->counts) HIPCHECK(e, hipMemcpy(io->counts, kws + o_cnt, (size_t)block_bytes, hipMemcpyDeviceToHost));
    io->ms[2] = wall();
    return VGX_OK;
}

// ---- who infects whom per time bin and variant class of many replicates (vgx_flows.hip, vgx_flows.h) ------------
// vgx_get_incidence step for step, with the block [n][T][P][P][V] and vgx_get_prevalence's variant_of in place of the mask: the
// host clock turns every replicate's times into T + 1 cuts, the device counts over the log in place in the form that fits, and
// the column summary reads the block where it lies.
extern "C" int vgx_get_flows(vgx_engine *e, vgx_flows_io *io) {
    if (!e || !io || io->n < 0 || (io->n > 0 && (!io->replicates || !io->outside))) return VGX_ERR_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    auto wall = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(); };
    io->passes = 0;
    io->form = 0;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    if (e->last_was_tau) return fail(e, VGX_ERR_ARG, "vgx_get_flows: the last call was vgx_simulate_tau (counts direct chains only)");
    if (!e->sc_host_valid || !e->dev_state_valid) return fail(e, VGX_ERR_ARG, "vgx_get_flows: needs a direct vgx_simulate_direct call with the event log first");
    if (!e->call_recorded) return fail(e, VGX_ERR_ARG, "vgx_get_flows: the last call did not record events");
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, T = io->T, V = io->V;
    if (T < 1 || T >= VGX_FLOW_MAX_BINS || !io->edges) return fail(e, VGX_ERR_ARG, "vgx_get_flows: T = " + std::to_string(T) + " bins: at least 1, below 2^24, with edges");
    for (int64_t k = 0; k <= T; k++) {
        if (!std::isfinite(io->edges[k])) return fail(e, VGX_ERR_ARG, "vgx_get_flows: edges[" + std::to_string(k) + "] is not finite");
        if (k > 0 && !(io->edges[k - 1] < io->edges[k]))
            return fail(e, VGX_ERR_ARG, "vgx_get_flows: edges must increase strictly (edges[" + std::to_string(k) + "])");
    }
    if (V < 1 || V > INT32_MAX || !io->variant_of) return fail(e, VGX_ERR_ARG, "vgx_get_flows: V = " + std::to_string(V) + " classes: at least 1, with variant_of");
    for (int64_t h = 0; h < H; h++)
        if (io->variant_of[h] < -1 || io->variant_of[h] >= V)
            return fail(e, VGX_ERR_ARG, "vgx_get_flows: variant_of[" + std::to_string(h) + "] = " + std::to_string(io->variant_of[h]) + " is outside [-1, " + std::to_string(V) + ")");
    int asked = VGX_FLOW_AUTO;
    if (const char *fm = getenv("VGX_FLOWS_FORM")) {
        if (!strcmp(fm, "dense")) asked = VGX_FLOW_DENSE;
        else if (!strcmp(fm, "split")) asked = VGX_FLOW_SPLIT;
        else if (*fm) return fail(e, VGX_ERR_ARG, std::string("vgx_get_flows: VGX_FLOWS_FORM=") + fm + " is neither dense nor split");
    }
    const int form = vgx_flow_form(asked, P, V);
    if (!form) {
        char why[256];
        vgx_flow_refusal(asked, P, V, why, sizeof why);
        return fail(e, VGX_ERR_ARG, std::string("vgx_get_flows: ") + why);
    }
    io->form = form;
    const int64_t cells = P * P * V;   // (P * V <= 2^14 and P <= 2^14: below 2^28)
    std::vector<int32_t> n_ev((size_t)n);
    {
        std::vector<char> seen((size_t)e->R, 0);
        for (int64_t i = 0; i < n; i++) {
            const int64_t r = io->replicates[i];
            if (r < 0 || r >= e->R) return fail(e, VGX_ERR_ARG, "vgx_get_flows: replicate index out of range");
            if (seen[(size_t)r]) return fail(e, VGX_ERR_ARG, "vgx_get_flows: replicates must be distinct");
            seen[(size_t)r] = 1;
            const VgxRepScalars &s = e->sc_host[(size_t)r];
            const int64_t first = s.restarts > 0 ? 0 : ((size_t)r < e->call_ev0.size() ? e->call_ev0[(size_t)r] : e->ev_ptr0);
            if (first != 0 || e->ev_base != 0)
                return fail(e, VGX_ERR_ARG, "vgx_get_flows: replicate " + std::to_string(r) + ": its chain does not start in the last call's device log (the model held " +
                                                std::to_string(e->ev_base != 0 ? e->ev_base : first) + " events when the ensemble started)");
            if (s.ev_ptr >= VGX_FLOW_MAX_EVENTS)
                return fail(e, VGX_ERR_ARG, "vgx_get_flows: replicate " + std::to_string(r) + " holds a chain of " + std::to_string(s.ev_ptr) + " events (2^30 or more)");
            if (s.ev_ptr < 0 || s.ev_ptr > e->evcap)
                return fail(e, VGX_ERR_ARG, "vgx_get_flows: event range of replicate " + std::to_string(r) + " outside the device log");
            n_ev[(size_t)i] = (int32_t)s.ev_ptr;
        }
    }
    if (n == 0) {
        io->ms[2] = wall();
        return VGX_OK;
    }
    int64_t tile = VGX_FLOW_TILE_DEFAULT;
    if (const char *tb = getenv("VGX_FLOWS_TILE_EVENTS")) tile = std::min<int64_t>(std::max<int64_t>(atoll(tb), 1), VGX_FLOW_MAX_EVENTS);
    HIPCHECK(e, hipSetDevice(e->device));
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    auto up8 = [](int64_t b) { return (b + 255) / 256 * 256; };
    auto dev_free = [](char *p) { (void)hipFree(p); };
    // what stays for the whole call: [rep | n_ev | cut | variant_of | counts]
    if (T * cells >= ((int64_t)1 << 40) / std::max<int64_t>(n, 1))
        return fail(e, VGX_ERR_ARG, "vgx_get_flows: the block of " + std::to_string(n) + " x " + std::to_string(T) + " x " + std::to_string(P) + " x " + std::to_string(P) +
                                        " x " + std::to_string(V) + " counts holds 2^40 cells or more: select fewer replicates per call");
    const int64_t block_bytes = n * T * cells * 4;
    const int64_t o_rep = 0, o_nev = o_rep + up8(n * 8), o_cut = o_nev + up8(n * 4), o_map = o_cut + up8(n * (T + 1) * 4),
                  o_cnt = o_map + up8(H * 4), keep_total = o_cnt + up8(block_bytes);
    if (keep_total > (int64_t)(free_b / 2))
        return fail(e, VGX_ERR_ARG, "vgx_get_flows: the block of " + std::to_string(n) + " x " + std::to_string(T) + " x " + std::to_string(P) + " x " + std::to_string(P) +
                                        " x " + std::to_string(V) + " counts and its cuts take " + std::to_string(keep_total) + " bytes, above half of the " +
                                        std::to_string((int64_t)free_b) + " bytes of free device memory: select fewer replicates per call");
    char *kws = nullptr;
    hipError_t er = hipMalloc((void **)&kws, (size_t)keep_total);
    if (er != hipSuccess) return fail(e, VGX_ERR_HIP, "vgx_get_flows: hipMalloc of " + std::to_string(keep_total) + " bytes: " + hipGetErrorString(er));
    std::unique_ptr<char, void (*)(char *)> khold(kws, dev_free);
    std::vector<int64_t> reps_all(io->replicates, io->replicates + n);
    HIPCHECK(e, hipMemcpyAsync(kws + o_rep, reps_all.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_nev, n_ev.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_map, io->variant_of, (size_t)H * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemsetAsync(kws + o_cnt, 0, (size_t)block_bytes, e->stream));   // zeroed once

    const int64_t share = (int64_t)(free_b / 2) - keep_total + 4096;
    std::vector<int32_t> cuts((size_t)(n * (T + 1)));
    const int rc_chunks = clock_chunks(e, "vgx_get_flows", reps_all, n_ev, (const int64_t *)(kws + o_rep), (const int32_t *)(kws + o_nev), share, io->ms,
        // host: a replicate's event times -> its T + 1 cuts
        [&](int64_t gi, const std::vector<double> &times) {
            int32_t *cut = cuts.data() + gi * (T + 1);
            VgxIncCutter ct{io->edges, T, cut};
            for (size_t k = 0; k < times.size(); k++) ct.event((int64_t)k, times[k]);
            ct.finish((int64_t)times.size());
            io->outside[2 * gi] = cut[0];
            io->outside[2 * gi + 1] = (int64_t)times.size() - cut[(size_t)T];
        },
        // device: the count of the chunk's replicates into their rows of the block
        [&](int64_t i0, int64_t i1, int64_t max_n) -> int {
            const int64_t m = i1 - i0;
            HIPCHECK(e, hipMemcpyAsync(kws + o_cut + i0 * (T + 1) * 4, cuts.data() + i0 * (T + 1), (size_t)(m * (T + 1)) * 4, hipMemcpyHostToDevice, e->stream));
            HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
            VgxFlowLaunch a{};
            a.m = m;
            a.log = (const int32_t *)e->r_evcols.p; a.evcap = e->evcap;
            a.rep = (const int64_t *)(kws + o_rep) + i0; a.n_ev = (const int32_t *)(kws + o_nev) + i0;
            a.cut = (const int32_t *)(kws + o_cut) + i0 * (T + 1);
            a.T = (int32_t)T; a.P = (int32_t)P; a.hapNum = (int32_t)H; a.V = (int32_t)V;
            a.variant_of = (const int32_t *)(kws + o_map);
            a.within = io->within ? 1 : 0; a.form = form;
            a.tile = (int32_t)tile; a.max_n = max_n;
            a.counts = (int32_t *)(kws + o_cnt) + i0 * T * cells;
            HIPCHECK(e, vgxi_flow_count(&a, e->stream));
            if (max_n > 0) io->passes += 1;
            HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
            if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)
                return fail(e, VGX_ERR_HIP, std::string("vgx_get_flows: counting kernel failed: ") + hipGetErrorString(er));
            float kms = 0.f;
            HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
            io->ms[0] += kms;
            return VGX_OK;
        });
    if (rc_chunks) return rc_chunks;
    if (io->summary) {
        char msg[512] = "";
        const int rc = vgxi_column_summary_i32("vgx_get_flows: summary", (const int32_t *)(kws + o_cnt), n, T * cells, io->summary, e->stream, msg, sizeof msg);
        if (rc) return fail(e, rc, msg);
    }
    if (io->counts) HIPCHECK(e, hipMemcpy(io->counts, kws + o_cnt, (size_t)block_bytes, hipMemcpyDeviceToHost));
    io->ms[2] = wall();
    return VGX_OK;
}

// ---- infectious hosts per variant class of many replicates at the times of one grid (vgx_prevalence.hip, vgx_prevalence.h)
// The split of vgx_get_incidence: the host clock turns every replicate's times into T + 2 bounds, the device forms the net change
// of every (interval, population, class) over the log in place and sums the intervals up per column; the column summary reads the
// values where they lie.
extern "C" int vgx_get_prevalence(vgx_engine *e, vgx_prevalence_io *io) {
    if (!e || !io || io->n < 0 || (io->n > 0 && (!io->replicates || !io->outside))) return VGX_ERR_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    auto wall = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(); };
    io->passes = 0;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    if (e->last_was_tau) return fail(e, VGX_ERR_ARG, "vgx_get_prevalence: the last call was vgx_simulate_tau (counts direct chains only)");
    if (!e->sc_host_valid || !e->dev_state_valid) return fail(e, VGX_ERR_ARG, "vgx_get_prevalence: needs a direct vgx_simulate_direct call with the event log first");
    if (!e->call_recorded) return fail(e, VGX_ERR_ARG, "vgx_get_prevalence: the last call did not record events");
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, T = io->T, V = io->V;
    if (T < 1 || T >= VGX_PREV_MAX_POINTS || !io->grid) return fail(e, VGX_ERR_ARG, "vgx_get_prevalence: T = " + std::to_string(T) + " grid points: at least 1, below 2^24, with grid");
    for (int64_t k = 0; k < T; k++) {
        if (!std::isfinite(io->grid[k])) return fail(e, VGX_ERR_ARG, "vgx_get_prevalence: grid[" + std::to_string(k) + "] is not finite");
        if (k > 0 && !(io->grid[k - 1] < io->grid[k]))
            return fail(e, VGX_ERR_ARG, "vgx_get_prevalence: grid must increase strictly (grid[" + std::to_string(k) + "])");
    }
    if (V < 1 || V > INT32_MAX || !io->variant_of) return fail(e, VGX_ERR_ARG, "vgx_get_prevalence: V = " + std::to_string(V) + " classes: at least 1, with variant_of");
    for (int64_t h = 0; h < H; h++)
        if (io->variant_of[h] < -1 || io->variant_of[h] >= V)
            return fail(e, VGX_ERR_ARG, "vgx_get_prevalence: variant_of[" + std::to_string(h) + "] = " + std::to_string(io->variant_of[h]) + " is outside [-1, " + std::to_string(V) + ")");
    for (int64_t pn = 0; pn < P; pn++)
        if (e->sizes[(size_t)pn] >= ((int64_t)1 << 31)) return fail(e, VGX_ERR_ARG, "vgx_get_prevalence: population sizes of 2^31 or more");
    if (vgx_prev_lds_bytes(P, V) > VGX_PREV_LDS_MAX)
        return fail(e, VGX_ERR_ARG, "vgx_get_prevalence: " + std::to_string(P) + " populations x " + std::to_string(V) + " classes need " + std::to_string(vgx_prev_lds_bytes(P, V)) +
                                        " bytes of cells, above the " + std::to_string((int64_t)VGX_PREV_LDS_MAX) + " bytes of LDS a counting workgroup may use");
    const int64_t cells = P * V;
    std::vector<int32_t> n_ev((size_t)n);
    {
        std::vector<char> seen((size_t)e->R, 0);
        for (int64_t i = 0; i < n; i++) {
            const int64_t r = io->replicates[i];
            if (r < 0 || r >= e->R) return fail(e, VGX_ERR_ARG, "vgx_get_prevalence: replicate index out of range");
            if (seen[(size_t)r]) return fail(e, VGX_ERR_ARG, "vgx_get_prevalence: replicates must be distinct");
            seen[(size_t)r] = 1;
            const VgxRepScalars &s = e->sc_host[(size_t)r];
            const int64_t first = s.restarts > 0 ? 0 : ((size_t)r < e->call_ev0.size() ? e->call_ev0[(size_t)r] : e->ev_ptr0);
            if (first != 0 || e->ev_base != 0)
                return fail(e, VGX_ERR_ARG, "vgx_get_prevalence: replicate " + std::to_string(r) + ": its chain does not start in the last call's device log (the model held " +
                                                std::to_string(e->ev_base != 0 ? e->ev_base : first) + " events when the ensemble started)");
            if (s.ev_ptr >= VGX_PREV_MAX_EVENTS)
                return fail(e, VGX_ERR_ARG, "vgx_get_prevalence: replicate " + std::to_string(r) + " holds a chain of " + std::to_string(s.ev_ptr) + " events (2^30 or more)");
            if (s.ev_ptr < 0 || s.ev_ptr > e->evcap)
                return fail(e, VGX_ERR_ARG, "vgx_get_prevalence: event range of replicate " + std::to_string(r) + " outside the device log");
            n_ev[(size_t)i] = (int32_t)s.ev_ptr;
        }
    }
    if (n == 0) {
        io->ms[2] = wall();
        return VGX_OK;
    }
    // the start of a chain folded through variant_of: the state the call started from, or the initial state after a restart
    std::vector<int32_t> start((size_t)(n * cells));
    {
        std::vector<int64_t> fold[2] = {std::vector<int64_t>((size_t)cells, 0), std::vector<int64_t>((size_t)cells, 0)};
        const std::vector<int64_t> *src[2] = {&e->hs.infectious, &e->hs.initial_infectious};
        for (int k = 0; k < 2; k++)
            for (int64_t pn = 0; pn < P; pn++)
                for (int64_t h = 0; h < H; h++)
                    if (io->variant_of[h] >= 0) fold[k][(size_t)(pn * V + io->variant_of[h])] += (*src[k])[(size_t)(pn * H + h)];
        for (int k = 0; k < 2; k++)
            for (int64_t c = 0; c < cells; c++)
                if (fold[k][(size_t)c] < 0 || fold[k][(size_t)c] > INT32_MAX) return fail(e, VGX_ERR_ARG, "vgx_get_prevalence: a start value outside [0, 2^31)");
        for (int64_t i = 0; i < n; i++) {
            const std::vector<int64_t> &f = fold[e->sc_host[(size_t)io->replicates[i]].restarts > 0 ? 1 : 0];
            for (int64_t c = 0; c < cells; c++) start[(size_t)(i * cells + c)] = (int32_t)f[(size_t)c];
        }
    }
    int64_t tile = VGX_PREV_TILE_DEFAULT;
    if (const char *tb = getenv("VGX_PREVALENCE_TILE_EVENTS")) tile = std::min<int64_t>(std::max<int64_t>(atoll(tb), 1), VGX_PREV_MAX_EVENTS);
    HIPCHECK(e, hipSetDevice(e->device));
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    auto up8 = [](int64_t b) { return (b + 255) / 256 * 256; };
    auto dev_free = [](char *p) { (void)hipFree(p); };
    // what stays for the whole call: [rep | n_ev | bound | variant_of | start | val | fin | min, max]
    const int64_t val_bytes = n * T * cells * 4, fin_bytes = n * cells * 4;
    const int64_t o_rep = 0, o_nev = o_rep + up8(n * 8), o_bnd = o_nev + up8(n * 4), o_map = o_bnd + up8(n * (T + 2) * 4), o_start = o_map + up8(H * 4),
                  o_val = o_start + up8(fin_bytes), o_fin = o_val + up8(val_bytes), o_mm = o_fin + up8(fin_bytes), keep_total = o_mm + 256;
    if (keep_total > (int64_t)(free_b / 2))
        return fail(e, VGX_ERR_ARG, "vgx_get_prevalence: the block of " + std::to_string(n) + " x " + std::to_string(T + 1) + " x " + std::to_string(P) + " x " + std::to_string(V) +
                                        " values (" + std::to_string(val_bytes + fin_bytes) + " bytes), its cuts and start take " + std::to_string(keep_total) +
                                        " bytes, above half of the " + std::to_string((int64_t)free_b) + " bytes of free device memory: select fewer replicates per call");
    char *kws = nullptr;
    hipError_t er = hipMalloc((void **)&kws, (size_t)keep_total);
    if (er != hipSuccess) return fail(e, VGX_ERR_HIP, "vgx_get_prevalence: hipMalloc of " + std::to_string(keep_total) + " bytes: " + hipGetErrorString(er));
    std::unique_ptr<char, void (*)(char *)> khold(kws, dev_free);
    std::vector<int64_t> reps_all(io->replicates, io->replicates + n);
    HIPCHECK(e, hipMemcpyAsync(kws + o_rep, reps_all.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_nev, n_ev.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_map, io->variant_of, (size_t)H * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_start, start.data(), (size_t)fin_bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemsetAsync(kws + o_val, 0, (size_t)(o_mm - o_val), e->stream));   // val and fin, zeroed once

    const int64_t share = (int64_t)(free_b / 2) - keep_total + 4096;
    std::vector<int32_t> bounds((size_t)(n * (T + 2)));
    const int rc_chunks = clock_chunks(e, "vgx_get_prevalence", reps_all, n_ev, (const int64_t *)(kws + o_rep), (const int32_t *)(kws + o_nev), share, io->ms,
        // host: a replicate's event times -> its T + 2 bounds
        [&](int64_t gi, const std::vector<double> &times) {
            int32_t *bound = bounds.data() + gi * (T + 2);
            VgxPrevCutter ct{io->grid, T, bound};
            for (size_t k = 0; k < times.size(); k++) ct.event((int64_t)k, times[k]);
            ct.finish((int64_t)times.size());
            io->outside[2 * gi] = bound[1];
            io->outside[2 * gi + 1] = (int64_t)times.size() - bound[(size_t)T];
        },
        // device: the net changes of the chunk's replicates into their rows of the block, then the running sums of those rows
        [&](int64_t i0, int64_t i1, int64_t max_n) -> int {
            const int64_t m = i1 - i0;
            HIPCHECK(e, hipMemcpyAsync(kws + o_bnd + i0 * (T + 2) * 4, bounds.data() + i0 * (T + 2), (size_t)(m * (T + 2)) * 4, hipMemcpyHostToDevice, e->stream));
            HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
            VgxPrevLaunch a{};
            a.m = m;
            a.log = (const int32_t *)e->r_evcols.p; a.evcap = e->evcap;
            a.rep = (const int64_t *)(kws + o_rep) + i0; a.n_ev = (const int32_t *)(kws + o_nev) + i0;
            a.bound = (const int32_t *)(kws + o_bnd) + i0 * (T + 2);
            a.T = (int32_t)T; a.P = (int32_t)P; a.hapNum = (int32_t)H; a.V = (int32_t)V;
            a.variant_of = (const int32_t *)(kws + o_map);
            a.tile = (int32_t)tile; a.max_n = max_n;
            a.val = (int32_t *)(kws + o_val) + i0 * T * cells;
            a.fin = (int32_t *)(kws + o_fin) + i0 * cells;
            a.start = (const int32_t *)(kws + o_start) + i0 * cells;
            HIPCHECK(e, vgxi_prev_count(&a, e->stream));
            if (max_n > 0) io->passes += 1;
            HIPCHECK(e, vgxi_prev_scan(&a, e->stream));
            HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
            if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)
                return fail(e, VGX_ERR_HIP, std::string("vgx_get_prevalence: counting or scan kernel failed: ") + hipGetErrorString(er));
            float kms = 0.f;
            HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
            io->ms[0] += kms;
            return VGX_OK;
        });
    if (rc_chunks) return rc_chunks;
    if (io->values) HIPCHECK(e, hipMemcpy(io->values, kws + o_val, (size_t)val_bytes, hipMemcpyDeviceToHost));
    if (io->final) HIPCHECK(e, hipMemcpy(io->final, kws + o_fin, (size_t)fin_bytes, hipMemcpyDeviceToHost));
    if (io->summary) {
        // the column summary sorts 32-bit keys of whole numbers in [0, 2^31)
        int32_t mm[2] = {0, 0};
        HIPCHECK(e, vgxi_prev_minmax((const int32_t *)(kws + o_val), n * T * cells, (int32_t *)(kws + o_mm), e->stream));
        HIPCHECK(e, hipMemcpyAsync(mm, kws + o_mm, sizeof mm, hipMemcpyDeviceToHost, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)
            return fail(e, VGX_ERR_HIP, std::string("vgx_get_prevalence: min/max kernel failed: ") + hipGetErrorString(er));
        if (mm[0] < 0)
            return fail(e, VGX_ERR_ARG, "vgx_get_prevalence: summary: a value of " + std::to_string(mm[0]) + " is not a whole number in [0, 2^31) (the log holds records outside the model)");
        char msg[512] = "";
        const int rc = vgxi_column_summary_i32("vgx_get_prevalence: summary", (const int32_t *)(kws + o_val), n, T * cells, io->summary, e->stream, msg, sizeof msg);
        if (rc) return fail(e, rc, msg);
    }
    io->ms[2] = wall();
    return VGX_OK;
}

// ---- ancestral lineages per variant class of many replicates at the times of one grid (vgx_lineages.hip, vgx_lineages.h)
// vgx_get_genealogies' walk and vgx_get_prevalence's grid in one call: the sizing kernel counts every chain's MUTATION and
// MIGRATION events, the host clock turns every replicate's times into T + 2 bounds, and pass by pass the device walks the selected
// replicates with the logging observer, bins their lineage logs into the block of net changes and sums the intervals up where
// they lie; the column summary reads the values there.  With `events` it is vgx_get_tree_events: the block is
// counts [n][T + 1][P][V][VGX_TE_K] behind io->values, binned by vgxi_te_bin, with no scan and no root.
static int lineages_call(vgx_engine *e, vgx_lineages_io *io, const bool events, const char *name) {
    if (io->n < 0 || (io->n > 0 && (!io->replicates || !io->rng_state || !io->status || !io->status_arg || !io->records || !io->rng_out)))
        return VGX_ERR_ARG;
    const std::string me = std::string(name) + ": ";
    const auto t_call = std::chrono::steady_clock::now();
    auto wall = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(); };
    io->passes = 0;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    io->kernel_ms[0] = io->kernel_ms[1] = io->kernel_ms[2] = 0.0;
    if (!e->sc_host_valid || !e->dev_state_valid) return fail(e, VGX_ERR_ARG, me + "no direct simulate call yet");
    if (e->last_was_tau) return fail(e, VGX_ERR_ARG, me + "the last call was vgx_simulate_tau (direct chains only)");
    if (!e->call_recorded) return fail(e, VGX_ERR_ARG, me + "the last call did not record events");
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, T = io->T, V = io->V;
    if (T < 1 || T >= VGX_PREV_MAX_POINTS || !io->grid) return fail(e, VGX_ERR_ARG, me + "T = " + std::to_string(T) + " grid points: at least 1, below 2^24, with grid");
    for (int64_t k = 0; k < T; k++) {
        if (!std::isfinite(io->grid[k])) return fail(e, VGX_ERR_ARG, me + "grid[" + std::to_string(k) + "] is not finite");
        if (k > 0 && !(io->grid[k - 1] < io->grid[k]))
            return fail(e, VGX_ERR_ARG, me + "grid must increase strictly (grid[" + std::to_string(k) + "])");
    }
    if (V < 1 || V > INT32_MAX || !io->variant_of) return fail(e, VGX_ERR_ARG, me + "V = " + std::to_string(V) + " classes: at least 1, with variant_of");
    for (int64_t h = 0; h < H; h++)
        if (io->variant_of[h] < -1 || io->variant_of[h] >= V)
            return fail(e, VGX_ERR_ARG, me + "variant_of[" + std::to_string(h) + "] = " + std::to_string(io->variant_of[h]) + " is outside [-1, " + std::to_string(V) + ")");
    if (vgx_prev_lds_bytes(P, V) > VGX_PREV_LDS_MAX)
        return fail(e, VGX_ERR_ARG, me + "" + std::to_string(P) + " populations x " + std::to_string(V) + " classes need " + std::to_string(vgx_prev_lds_bytes(P, V)) +
                                        " bytes of cells, above the " + std::to_string((int64_t)VGX_PREV_LDS_MAX) + " bytes of LDS a counting workgroup may use");
    if (events && vgx_te_lds_bytes(P, V) > VGX_PREV_LDS_MAX)
        return fail(e, VGX_ERR_ARG, me + std::to_string(P) + " populations x " + std::to_string(V) + " classes x " + std::to_string(VGX_TE_K) + " channels need " +
                                        std::to_string(vgx_te_lds_bytes(P, V)) + " bytes of cells, above the " + std::to_string((int64_t)VGX_PREV_LDS_MAX) +
                                        " bytes of LDS a counting workgroup may use");
    // the block: lineages' [n][T][cells] values and [n][cells] root, or the events' [n][T + 1][cells] counts with no root
    const int64_t cells = events ? P * V * VGX_TE_K : P * V, rows = events ? T + 1 : T;
    std::vector<int32_t> n_ev((size_t)n);
    std::vector<int64_t> n_ev64((size_t)n), sC((size_t)n);
    {
        std::vector<char> seen((size_t)e->R, 0);
        for (int64_t i = 0; i < n; i++) {
            const int64_t r = io->replicates[i];
            if (r < 0 || r >= e->R) return fail(e, VGX_ERR_ARG, me + "replicate index out of range");
            if (seen[(size_t)r]) return fail(e, VGX_ERR_ARG, me + "replicates must be distinct");
            seen[(size_t)r] = 1;
            const VgxRepScalars &s = e->sc_host[(size_t)r];
            const int64_t first = s.restarts > 0 ? 0 : ((size_t)r < e->call_ev0.size() ? e->call_ev0[(size_t)r] : e->ev_ptr0);
            if (first != 0 || e->ev_base != 0)
                return fail(e, VGX_ERR_ARG, me + "the chain of replicate " + std::to_string(r) +
                                                " does not start in the last call's device log (events.ptr was not 0 at its start)");
            if (s.ev_ptr >= VGX_PREV_MAX_EVENTS)
                return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + " holds a chain of " + std::to_string(s.ev_ptr) + " events (2^30 or more)");
            if (s.ev_ptr < 0 || s.ev_ptr > e->evcap)
                return fail(e, VGX_ERR_ARG, me + "event range of replicate " + std::to_string(r) + " outside the device log");
            n_ev[(size_t)i] = (int32_t)s.ev_ptr;
            n_ev64[(size_t)i] = s.ev_ptr;
            sC[(size_t)i] = s.sCounter;
        }
    }
    if (n == 0) {
        io->ms[2] = wall();
        return VGX_OK;
    }
    int64_t tile = VGX_LN_TILE_DEFAULT;
    if (const char *tb = getenv("VGX_LINEAGES_TILE_RECORDS")) tile = std::min<int64_t>(std::max<int64_t>(atoll(tb), 1), VGX_PREV_MAX_EVENTS);
    HIPCHECK(e, hipSetDevice(e->device));
    const int32_t *log = (const int32_t *)e->r_evcols.p;
    // the walk reads the 8-byte counts of the final occupancy lists
    if (!e->counts64_valid) {
        HIPCHECK(e, vgxi_launch_counts64(e->dr.lcnt32, e->dr.lcnt, e->R * P * e->cap, e->stream));
        HIPCHECK(e, hipStreamSynchronize(e->stream));
        e->counts64_valid = true;
    }
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    auto up8 = [](int64_t b) { return (b + 255) / 256 * 256; };
    auto dev_free = [](char *p) { (void)hipFree(p); };
    // what stays for the whole call: [rep | n_ev | n_ev (8 bytes) | event counts | bound | variant_of | val | fin | min, max]
    const int64_t val_bytes = n * rows * cells * 4, fin_bytes = events ? 0 : n * cells * 4;
    const int64_t o_rep = 0, o_nev = o_rep + up8(n * 8), o_nev64 = o_nev + up8(n * 4), o_cnt = o_nev64 + up8(n * 8), o_bnd = o_cnt + up8(n * 16),
                  o_map = o_bnd + up8(n * (T + 2) * 4), o_val = o_map + up8(H * 4), o_fin = o_val + up8(val_bytes), o_mm = o_fin + up8(fin_bytes),
                  keep_total = o_mm + 256;
    if (keep_total > (int64_t)(free_b / 2))
        return fail(e, VGX_ERR_ARG, me + "the block of " + std::to_string(n) + " x " + std::to_string(T + 1) + " x " + std::to_string(P) + " x " + std::to_string(V) +
                                        " values (" + std::to_string(val_bytes + fin_bytes) + " bytes) and its cuts take " + std::to_string(keep_total) +
                                        " bytes, above half of the " + std::to_string((int64_t)free_b) + " bytes of free device memory: select fewer replicates per call");
    char *kws = nullptr;
    hipError_t er = hipMalloc((void **)&kws, (size_t)keep_total);
    if (er != hipSuccess) return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(keep_total) + " bytes: " + hipGetErrorString(er));
    std::unique_ptr<char, void (*)(char *)> khold(kws, dev_free);
    std::vector<int64_t> reps_all(io->replicates, io->replicates + n);
    HIPCHECK(e, hipMemcpyAsync(kws + o_rep, reps_all.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_nev, n_ev.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_nev64, n_ev64.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_map, io->variant_of, (size_t)H * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemsetAsync(kws + o_val, 0, (size_t)(o_mm - o_val), e->stream));   // val and fin, zeroed once
    // the MUTATION and MIGRATION events of every chain: the capacity of its lineage log
    std::vector<int64_t> cnt((size_t)n * 2);
    HIPCHECK(e, vgxi_gw_count(log, e->evcap, (const int64_t *)(kws + o_rep), (const int64_t *)(kws + o_nev64), n, (int64_t *)(kws + o_cnt), e->stream));
    HIPCHECK(e, hipMemcpyAsync(cnt.data(), kws + o_cnt, (size_t)n * 16, hipMemcpyDeviceToHost, e->stream));
    if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)
        return fail(e, VGX_ERR_HIP, std::string(me + "counting pass: ") + hipGetErrorString(er));

    // host: every replicate's event times -> its T + 2 bounds (the device work of a clock chunk comes later, pass by pass)
    const int64_t share_clock = (int64_t)(free_b / 2) - keep_total + 4096;
    std::vector<int32_t> bounds((size_t)(n * (T + 2)));
    const int rc_chunks = clock_chunks(e, "vgx_get_lineages", reps_all, n_ev, (const int64_t *)(kws + o_rep), (const int32_t *)(kws + o_nev), share_clock, io->ms,
        [&](int64_t gi, const std::vector<double> &times) {
            VgxPrevCutter ct{io->grid, T, bounds.data() + gi * (T + 2)};
            for (size_t k = 0; k < times.size(); k++) ct.event((int64_t)k, times[k]);
            ct.finish((int64_t)times.size());
        },
        [&](int64_t, int64_t, int64_t) -> int { return VGX_OK; });
    if (rc_chunks) return rc_chunks;
    HIPCHECK(e, hipMemcpyAsync(kws + o_bnd, bounds.data(), bounds.size() * 4, hipMemcpyHostToDevice, e->stream));

    // per-replicate workspace (elements), and the passes: every pass holds at most `share` bytes
    std::vector<VgxLnDesc> desc((size_t)n);
    std::vector<int64_t> bytes((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        VgxLnDesc &d = desc[(size_t)i];
        d.rep = io->replicates[i];
        d.n_ev = n_ev64[(size_t)i];
        d.sCounter = sC[(size_t)i];
        d.tsize = d.sCounter >= 2 ? vgx_gw_table_size(d.n_ev, P * H) : 0;
        d.arena_cap = d.sCounter >= 2 ? d.n_ev : 0;
        d.rec_cap = vgx_ln_capacity(d.sCounter, cnt[(size_t)(2 * i)], cnt[(size_t)(2 * i + 1)]);
        for (int k = 0; k < 4; k++) d.rng[k] = io->rng_state[i * 4 + k];
        const int64_t nodes = d.sCounter >= 2 ? 2 * d.sCounter - 1 : 0;
        bytes[(size_t)i] = d.tsize * 28 + d.arena_cap * 4 + nodes * 4 + d.rec_cap * 24 + (int64_t)sizeof(VgxLnDesc) + 80;
    }
    int64_t share = std::max<int64_t>((int64_t)(free_b / 2) - keep_total, 1);
    if (const char *cb = getenv("VGX_GENEALOGY_CHUNK_BYTES")) share = std::min<int64_t>(share, std::max<int64_t>(atoll(cb), 1));
    struct Events {   // the stages of a pass, timed apart
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        ~Events() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
    } tm;
    for (hipEvent_t &x : tm.ev) HIPCHECK(e, hipEventCreate(&x));
    int64_t i0 = 0;
    while (i0 < n) {
        int64_t i1 = i0, sum = 0;
        while (i1 < n && (i1 == i0 || sum + bytes[(size_t)i1] <= share)) sum += bytes[(size_t)i1++];
        const int64_t m = i1 - i0;
        int64_t TB = 0, A = 0, N = 0, Rc = 0, max_rec = 0;
        std::vector<VgxLnDesc> dp(desc.begin() + i0, desc.begin() + i1);
        for (int64_t j = 0; j < m; j++) {
            VgxLnDesc &d = dp[(size_t)j];
            d.tab_off = TB; d.arena_off = A; d.node_off = N; d.rec_off = Rc;
            TB += d.tsize; A += d.arena_cap; N += d.sCounter >= 2 ? 2 * d.sCounter - 1 : 0; Rc += d.rec_cap;
            max_rec = std::max<int64_t>(max_rec, d.rec_cap);
        }
        // one allocation: [desc | res | rng | n_rec | key | cnt | base | len | lcap | arena | parents | lineage logs]
        const int64_t o_desc = 0, o_res = o_desc + up8(m * (int64_t)sizeof(VgxLnDesc)), o_rng = o_res + up8(m * 40), o_nrec = o_rng + up8(m * 32),
                      o_key = o_nrec + up8(m * 8), o_tcnt = o_key + up8(TB * 8), o_base = o_tcnt + up8(TB * 8), o_len = o_base + up8(TB * 4),
                      o_lcap = o_len + up8(TB * 4), o_arena = o_lcap + up8(TB * 4), o_tree = o_arena + up8(A * 4), o_rec = o_tree + up8(N * 4),
                      total = o_rec + up8(Rc * 24);
        char *ws = nullptr;
        er = hipMalloc((void **)&ws, (size_t)total);
        if (er != hipSuccess)
            return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(total) + " bytes: " + hipGetErrorString(er));
        std::unique_ptr<char, void (*)(char *)> hold(ws, dev_free);
        VgxLnLaunch a{};
        a.m = m;
        a.desc = (const VgxLnDesc *)(ws + o_desc);
        a.log = log; a.evcap = e->evcap;
        a.nocc = e->dr.nocc; a.lhap = e->dr.lhap; a.lcnt = e->dr.lcnt;
        a.P = P; a.H = H; a.cap = e->cap;
        a.key = (int64_t *)(ws + o_key); a.cnt = (int64_t *)(ws + o_tcnt);
        a.base = (int32_t *)(ws + o_base); a.len = (int32_t *)(ws + o_len); a.lcap = (int32_t *)(ws + o_lcap);
        a.arena = (int32_t *)(ws + o_arena);
        a.tree = (int32_t *)(ws + o_tree);
        a.rec = (int32_t *)(ws + o_rec);
        a.res = (int64_t *)(ws + o_res);
        a.rng_out = (uint64_t *)(ws + o_rng);
        a.n_rec = (int64_t *)(ws + o_nrec);
        a.bound = (const int32_t *)(kws + o_bnd) + i0 * (T + 2);
        a.T = (int32_t)T; a.V = (int32_t)V;
        a.variant_of = (const int32_t *)(kws + o_map);
        a.tile = (int32_t)tile; a.max_rec = max_rec;
        a.val = (int32_t *)(kws + o_val) + i0 * rows * cells;
        a.fin = (int32_t *)(kws + o_fin) + i0 * cells;
        HIPCHECK(e, hipMemcpyAsync(ws + o_desc, dp.data(), (size_t)m * sizeof(VgxLnDesc), hipMemcpyHostToDevice, e->stream));
        if (TB > 0) HIPCHECK(e, hipMemsetAsync(a.key, 0xFF, (size_t)TB * 8, e->stream));   // every slot empty (-1)
        HIPCHECK(e, hipEventRecord(tm.ev[0], e->stream));
        HIPCHECK(e, vgxi_ln_walk(&a, e->stream));
        HIPCHECK(e, hipEventRecord(tm.ev[1], e->stream));
        if (events) {
            const VgxTeLaunch b{m, a.desc, a.rec, a.n_rec, a.bound, a.T, (int32_t)P, (int32_t)H, a.V, a.variant_of, a.tile, max_rec, a.val};
            HIPCHECK(e, vgxi_te_bin(&b, e->stream));
        } else {
            HIPCHECK(e, vgxi_ln_bin(&a, e->stream));
        }
        HIPCHECK(e, hipEventRecord(tm.ev[2], e->stream));
        if (!events) HIPCHECK(e, vgxi_ln_scan(&a, e->stream));
        HIPCHECK(e, hipEventRecord(tm.ev[3], e->stream));
        std::vector<int64_t> res((size_t)m * 5), nrec((size_t)m);
        HIPCHECK(e, hipMemcpyAsync(res.data(), a.res, (size_t)m * 40, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->rng_out + i0 * 4, a.rng_out, (size_t)m * 32, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(nrec.data(), a.n_rec, (size_t)m * 8, hipMemcpyDeviceToHost, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)   // before anything reads the outputs
            return fail(e, VGX_ERR_HIP, std::string(me + "walk, binning or scan kernel failed: ") + hipGetErrorString(er));
        for (int k = 0; k < 3; k++) {
            float kms = 0.f;
            HIPCHECK(e, hipEventElapsedTime(&kms, tm.ev[k], tm.ev[k + 1]));
            io->kernel_ms[k] += kms;
            io->ms[0] += kms;
        }
        for (int64_t j = 0; j < m; j++) {
            io->status[i0 + j] = res[(size_t)(j * 5)];
            io->status_arg[i0 + j] = res[(size_t)(j * 5 + 1)];
            io->records[i0 + j] = nrec[(size_t)j];
        }
        io->passes += 1;
        i0 = i1;
    }
    if (io->values) HIPCHECK(e, hipMemcpy(io->values, kws + o_val, (size_t)val_bytes, hipMemcpyDeviceToHost));
    if (!events) HIPCHECK(e, hipMemcpy(io->root, kws + o_fin, (size_t)fin_bytes, hipMemcpyDeviceToHost));
    if (io->summary) {
        if (!io->summary->group_of) return fail(e, VGX_ERR_ARG, me + "summary: null group_of");
        int64_t failed = 0;
        for (int64_t i = 0; i < n; i++) failed += io->summary->group_of[i] >= 0 && io->status[i] != VGX_GW_OK;
        if (failed > 0)
            return fail(e, VGX_ERR_ARG, me + "summary: " + std::to_string(failed) + " replicate(s) of a group have a walk that failed (status is not 0): leave them out of the groups");
        // the column summary sorts 32-bit keys of whole numbers in [0, 2^31)
        int32_t mm[2] = {0, 0};
        HIPCHECK(e, vgxi_prev_minmax((const int32_t *)(kws + o_val), n * rows * cells, (int32_t *)(kws + o_mm), e->stream));
        HIPCHECK(e, hipMemcpyAsync(mm, kws + o_mm, sizeof mm, hipMemcpyDeviceToHost, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)
            return fail(e, VGX_ERR_HIP, std::string(me + "min/max kernel failed: ") + hipGetErrorString(er));
        if (mm[0] < 0)
            return fail(e, VGX_ERR_ARG, me + "summary: a value of " + std::to_string(mm[0]) + " is not a whole number in [0, 2^31)");
        char msg[512] = "";
        const int rc = vgxi_column_summary_i32((me + "summary").c_str(), (const int32_t *)(kws + o_val), n, rows * cells, io->summary, e->stream, msg, sizeof msg);
        if (rc) return fail(e, rc, msg);
    }
    io->ms[2] = wall();
    return VGX_OK;
}

extern "C" int vgx_get_lineages(vgx_engine *e, vgx_lineages_io *io) {
    if (!e || !io || (io->n > 0 && !io->root)) return VGX_ERR_ARG;
    return lineages_call(e, io, false, "vgx_get_lineages");
}

// ---- coalescences, samples, mutations and moves of the trees per interval (vgx_tree_events.hip, vgx_tree_events.h) ----
// vgx_get_lineages with the kinds kept apart: the same checks, sizing, cuts, passes and walk; the binning kernel of
// vgx_tree_events.hip counts every pass's logs into the block [n][T + 1][P][V][VGX_TE_K] and no scan follows.
extern "C" int vgx_get_tree_events(vgx_engine *e, vgx_tree_events_io *io) {
    if (!e || !io) return VGX_ERR_ARG;
    vgx_lineages_io l{};
    l.n = io->n; l.replicates = io->replicates; l.rng_state = io->rng_state;
    l.T = io->T; l.grid = io->grid; l.V = io->V; l.variant_of = io->variant_of;
    l.values = io->counts;
    l.status = io->status; l.status_arg = io->status_arg; l.records = io->records; l.rng_out = io->rng_out;
    l.summary = io->summary;
    const int rc = lineages_call(e, &l, true, "vgx_get_tree_events");
    io->passes = l.passes;
    for (int k = 0; k < 3; k++) io->ms[k] = l.ms[k];
    io->kernel_ms[0] = l.kernel_ms[0]; io->kernel_ms[1] = l.kernel_ms[1];
    return rc;
}

// ---- balance, depth and branch statistics of every tree (vgx_tree_shapes.hip, vgx_tree_shape.h) ----------------------
// The walk pass of vgx_get_genealogies with the conversion left out: of the walk's outputs only the node event indices come to the
// host, the host clock turns them into node times (the lookup of vgx_get_genealogies), the times go back and the shape kernel reduces
// every tree where the walk left it.
extern "C" int vgx_get_tree_shapes(vgx_engine *e, vgx_tree_shapes_io *io) {
    if (!e || !io || io->n < 0 ||
        (io->n > 0 && (!io->replicates || !io->rng_state || !io->stats || !io->lengths || !io->status || !io->status_arg || !io->rng_out)))
        return VGX_ERR_ARG;
    const std::string me = "vgx_get_tree_shapes: ";
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
    io->passes = 0;
    io->ms[0] = io->ms[1] = io->ms[2] = io->ms[3] = 0.0;
    if (!e->sc_host_valid || !e->dev_state_valid) return fail(e, VGX_ERR_ARG, me + "no direct simulate call yet");
    if (e->last_was_tau) return fail(e, VGX_ERR_ARG, me + "the last call was vgx_simulate_tau (direct chains only)");
    if (!e->call_recorded) return fail(e, VGX_ERR_ARG, me + "the last call did not record events");
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum;
    std::vector<int64_t> n_ev((size_t)n), sC((size_t)n);
    {
        std::vector<char> seen((size_t)e->R, 0);
        for (int64_t i = 0; i < n; i++) {
            const int64_t r = io->replicates[i];
            if (r < 0 || r >= e->R) return fail(e, VGX_ERR_ARG, me + "replicate index out of range");
            if (seen[(size_t)r]) return fail(e, VGX_ERR_ARG, me + "replicates must be distinct");
            seen[(size_t)r] = 1;
            const VgxRepScalars &s = e->sc_host[(size_t)r];
            const int64_t first = s.restarts > 0 ? 0 : ((size_t)r < e->call_ev0.size() ? e->call_ev0[(size_t)r] : e->ev_ptr0);
            if (first != 0 || e->ev_base != 0)
                return fail(e, VGX_ERR_ARG, me + "the chain of replicate " + std::to_string(r) +
                                                " does not start in the last call's device log (events.ptr was not 0 at its start)");
            if (s.ev_ptr < 0 || s.ev_ptr > e->evcap || s.ev_ptr >= ((int64_t)1 << 30))
                return fail(e, VGX_ERR_ARG, me + "event range of replicate " + std::to_string(r) + " outside the device log");
            n_ev[(size_t)i] = s.ev_ptr;
            sC[(size_t)i] = s.sCounter;
        }
    }
    if (n == 0) {
        io->ms[3] = since(t_call);
        return VGX_OK;
    }
    HIPCHECK(e, hipSetDevice(e->device));
    const int32_t *log = (const int32_t *)e->r_evcols.p;
    auto up8 = [](int64_t b) { return (b + 255) / 256 * 256; };
    hipError_t er;
    // the MUTATION and MIGRATION events of every chain: the record capacities the walk needs (what the sizing call of vgx_get_genealogies counts)
    std::vector<int64_t> cnt((size_t)n * 2);
    {
        char *cws = nullptr;
        const int64_t o_n = up8(n * 8), o_out = o_n + up8(n * 8);
        if ((er = hipMalloc((void **)&cws, (size_t)(o_out + up8(n * 16)))) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "hipMalloc: " + hipGetErrorString(er));
        std::unique_ptr<char, void (*)(char *)> chold(cws, [](char *p) { (void)hipFree(p); });
        HIPCHECK(e, hipMemcpyAsync(cws, io->replicates, (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(cws + o_n, n_ev.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, vgxi_gw_count(log, e->evcap, (const int64_t *)cws, (const int64_t *)(cws + o_n), n, (int64_t *)(cws + o_out), e->stream));
        HIPCHECK(e, hipMemcpyAsync(cnt.data(), cws + o_out, (size_t)n * 16, hipMemcpyDeviceToHost, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "counting pass: " + hipGetErrorString(er));
    }
    // the walk reads the 8-byte counts of the final occupancy lists
    if (!e->counts64_valid) {
        HIPCHECK(e, vgxi_launch_counts64(e->dr.lcnt32, e->dr.lcnt, e->R * P * e->cap, e->stream));
        HIPCHECK(e, hipStreamSynchronize(e->stream));
        e->counts64_valid = true;
    }
    // per-replicate workspace and outputs (elements), and the passes: every pass holds at most `share` bytes
    std::vector<VgxGwDesc> desc((size_t)n);
    std::vector<int64_t> bytes((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        VgxGwDesc &d = desc[(size_t)i];
        const int64_t nodes = sC[(size_t)i] >= 2 ? 2 * sC[(size_t)i] - 1 : 0;
        d.rep = io->replicates[i];
        d.n_ev = n_ev[(size_t)i];
        d.sCounter = sC[(size_t)i];
        d.tsize = d.sCounter >= 2 ? vgx_gw_table_size(d.n_ev, P * H) : 0;
        d.arena_cap = d.sCounter >= 2 ? d.n_ev : 0;
        d.mut_cap = cnt[(size_t)(2 * i)];
        d.mig_cap = cnt[(size_t)(2 * i + 1)] + nodes;
        for (int k = 0; k < 4; k++) d.rng[k] = io->rng_state[i * 4 + k];
        bytes[(size_t)i] = d.tsize * 28 + d.arena_cap * 4 + nodes * (12 + 8 + VGX_TS_NODE_BYTES) + d.mut_cap * 20 + d.mig_cap * 16 +
                           (int64_t)(sizeof(VgxGwDesc) + sizeof(VgxTsDesc)) + 72 + 8 * (VGX_TS_K + VGX_TS_L + 2);
    }
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    int64_t share = (int64_t)(free_b / 2);
    if (const char *cb = getenv("VGX_GENEALOGY_CHUNK_BYTES")) share = std::min<int64_t>(share, std::max<int64_t>(atoll(cb), 1));
    std::vector<int64_t> mism((size_t)n, 0);
    int64_t i0 = 0;
    while (i0 < n) {
        int64_t i1 = i0, sum = 0;
        while (i1 < n && (i1 == i0 || sum + bytes[(size_t)i1] <= share)) sum += bytes[(size_t)i1++];
        const int64_t m = i1 - i0;
        int64_t T = 0, A = 0, N = 0, M = 0, G = 0;
        std::vector<VgxGwDesc> dp(desc.begin() + i0, desc.begin() + i1);
        std::vector<VgxTsDesc> ts((size_t)m);
        for (int64_t j = 0; j < m; j++) {
            VgxGwDesc &d = dp[(size_t)j];
            const int64_t nodes = d.sCounter >= 2 ? 2 * d.sCounter - 1 : 0;
            d.tab_off = T; d.arena_off = A; d.node_off = N; d.mut_off = M; d.mig_off = G;
            ts[(size_t)j] = VgxTsDesc{N, nodes};
            T += d.tsize; A += d.arena_cap; N += nodes; M += d.mut_cap; G += d.mig_cap;
        }
        // one allocation: the walk's of vgx_get_genealogies [desc | res | rng | key | cnt | base | len | lcap | arena | node x3 | mut x5 | mig x4],
        // then [tree descs | node times | A, B | seven int32 accumulators | stats | lengths | status]
        const int64_t o_desc = 0, o_res = o_desc + up8(m * (int64_t)sizeof(VgxGwDesc)), o_rng = o_res + up8(m * 40),
                      o_key = o_rng + up8(m * 32), o_cnt = o_key + up8(T * 8), o_base = o_cnt + up8(T * 8), o_len = o_base + up8(T * 4),
                      o_lcap = o_len + up8(T * 4), o_arena = o_lcap + up8(T * 4), o_out = o_arena + up8(A * 4),
                      o_ts = o_out + up8((3 * N + 5 * M + 4 * G) * 4), o_times = o_ts + up8(m * (int64_t)sizeof(VgxTsDesc)), o_w64 = o_times + up8(N * 8),
                      o_w32 = o_w64 + up8(2 * N * 8), o_stats = o_w32 + up8(7 * N * 4), o_lens = o_stats + up8(m * VGX_TS_K * 8),
                      o_status = o_lens + up8(m * VGX_TS_L * 8), total = o_status + up8(m * 16);
        char *ws = nullptr;
        if ((er = hipMalloc((void **)&ws, (size_t)total)) != hipSuccess)
            return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(total) + " bytes: " + hipGetErrorString(er));
        std::unique_ptr<char, void (*)(char *)> hold(ws, [](char *p) { (void)hipFree(p); });
        VgxGwLaunch a{};
        a.n = m;
        a.desc = (const VgxGwDesc *)(ws + o_desc);
        a.log = log; a.evcap = e->evcap;
        a.nocc = e->dr.nocc; a.lhap = e->dr.lhap; a.lcnt = e->dr.lcnt;
        a.P = P; a.H = H; a.cap = e->cap;
        a.key = (int64_t *)(ws + o_key); a.cnt = (int64_t *)(ws + o_cnt);
        a.base = (int32_t *)(ws + o_base); a.len = (int32_t *)(ws + o_len); a.lcap = (int32_t *)(ws + o_lcap);
        a.arena = (int32_t *)(ws + o_arena);
        int32_t *o32 = (int32_t *)(ws + o_out);
        a.tree = o32; a.tree_pop = o32 + N; a.node_ev = o32 + 2 * N;
        int32_t *mu = o32 + 3 * N;
        a.mut_node = mu; a.mut_AS = mu + M; a.mut_DS = mu + 2 * M; a.mut_site = mu + 3 * M; a.mut_ev = mu + 4 * M;
        int32_t *mg = mu + 5 * M;
        a.mig_node = mg; a.mig_old = mg + G; a.mig_new = mg + 2 * G; a.mig_ev = mg + 3 * G;
        a.res = (int64_t *)(ws + o_res);
        a.rng_out = (uint64_t *)(ws + o_rng);
        // 1. the walk, in wave layout
        HIPCHECK(e, hipMemcpyAsync(ws + o_desc, dp.data(), (size_t)m * sizeof(VgxGwDesc), hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(ws + o_ts, ts.data(), (size_t)m * sizeof(VgxTsDesc), hipMemcpyHostToDevice, e->stream));
        if (T > 0) HIPCHECK(e, hipMemsetAsync(a.key, 0xFF, (size_t)T * 8, e->stream));   // every slot empty (-1)
        HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
        HIPCHECK(e, vgxi_gw_walk(&a, 1, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        // 2. before anything reads the walk's outputs
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "walk kernel failed: " + hipGetErrorString(er));
        float kms = 0.f;
        HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
        io->ms[0] += kms;
        std::vector<int64_t> res((size_t)m * 5);
        HIPCHECK(e, hipMemcpy(res.data(), a.res, (size_t)m * 40, hipMemcpyDeviceToHost));
        HIPCHECK(e, hipMemcpy(io->rng_out + i0 * 4, a.rng_out, (size_t)m * 32, hipMemcpyDeviceToHost));
        // 3. the node event indices alone  4. every replicate's host clock  5. the node times, back to the device
        const auto t_clock = std::chrono::steady_clock::now();
        std::vector<int32_t> h_nev((size_t)N);
        std::vector<double> h_times((size_t)N, 0.0);
        if (N > 0) HIPCHECK(e, hipMemcpy(h_nev.data(), a.node_ev, (size_t)N * 4, hipMemcpyDeviceToHost));
        std::vector<std::string> errs((size_t)m);
        std::vector<int> rcs((size_t)m, 0);
        int64_t work = 0;
        for (int64_t j = 0; j < m; j++) work += dp[(size_t)j].n_ev;
        for_parts(m, [&](int64_t j0, int64_t j1, unsigned) {
            if (hipSetDevice(e->device) != hipSuccess) { for (int64_t j = j0; j < j1; j++) { rcs[(size_t)j] = VGX_ERR_HIP; errs[(size_t)j] = "hipSetDevice"; } return; }
            vgx_engine::HostClock hc;
            for (int64_t j = j0; j < j1; j++) {
                const VgxGwDesc &d = dp[(size_t)j];
                int rc = clock_build(e, d.rep, hc, errs[(size_t)j]);
                if (rc) { rcs[(size_t)j] = rc; continue; }
                mism[(size_t)(i0 + j)] = hc.limit_mismatch ? 1 : 0;
                if (res[(size_t)(j * 5)] != VGX_GW_OK) continue;
                bool ok = true;
                const int64_t nodes = 2 * d.sCounter - 1;
                for (int64_t k = 0; k < nodes; k++) {   // (the lookup of vgx_get_genealogies: -1 = 0.0)
                    const int32_t ev = h_nev[(size_t)(d.node_off + k)];
                    const int64_t q = (int64_t)ev - hc.e0;
                    if (ev < 0) h_times[(size_t)(d.node_off + k)] = 0.0;
                    else if (q < 0 || q >= (int64_t)hc.times.size()) ok = false;
                    else h_times[(size_t)(d.node_off + k)] = hc.times[(size_t)q];
                }
                if (!ok) { rcs[(size_t)j] = VGX_ERR_ARG; errs[(size_t)j] = me + "an event index outside the host clock's range"; }
            }
        }, std::max<int64_t>(work / std::max<int64_t>(m, 1), 1) * 64);
        for (int64_t j = 0; j < m; j++)
            if (rcs[(size_t)j]) return fail(e, rcs[(size_t)j], errs[(size_t)j]);
        if (N > 0) HIPCHECK(e, hipMemcpy(ws + o_times, h_times.data(), (size_t)N * 8, hipMemcpyHostToDevice));
        io->ms[2] += since(t_clock);
        // 6. the shape kernel
        VgxTsLaunch b{};
        b.n = m;
        b.desc = (const VgxTsDesc *)(ws + o_ts);
        b.res = a.res;
        b.tree = a.tree; b.node_ev = a.node_ev; b.times = (const double *)(ws + o_times);
        int32_t *w32 = (int32_t *)(ws + o_w32);
        int64_t *w64 = (int64_t *)(ws + o_w64);
        b.w = VgxTsWork{w32, w32 + N, w32 + 2 * N, w32 + 3 * N, w32 + 4 * N, w32 + 5 * N, w32 + 6 * N, w64, w64 + N};
        b.stats = (int64_t *)(ws + o_stats); b.lengths = (double *)(ws + o_lens); b.status = (int64_t *)(ws + o_status);
        HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
        HIPCHECK(e, vgxi_ts_shape(&b, e->stream));
        HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
        // 7. before anything reads the rows
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "shape kernel failed: " + hipGetErrorString(er));
        HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
        io->ms[1] += kms;
        std::vector<int64_t> st2((size_t)m * 2);
        HIPCHECK(e, hipMemcpy(io->stats + i0 * VGX_TS_K, b.stats, (size_t)m * VGX_TS_K * 8, hipMemcpyDeviceToHost));
        HIPCHECK(e, hipMemcpy(io->lengths + i0 * VGX_TS_L, b.lengths, (size_t)m * VGX_TS_L * 8, hipMemcpyDeviceToHost));
        HIPCHECK(e, hipMemcpy(st2.data(), b.status, (size_t)m * 16, hipMemcpyDeviceToHost));
        for (int64_t j = 0; j < m; j++) {
            io->status[i0 + j] = st2[(size_t)(2 * j)];
            io->status_arg[i0 + j] = st2[(size_t)(2 * j + 1)];
        }
        io->passes += 1;
        i0 = i1;
    }
    // every replicate's clock was built once, as when the replicates are fetched one by one
    for (int64_t i = 0; i < n; i++) e->clock_mismatches += mism[(size_t)i];
    io->ms[3] = since(t_call);
    return VGX_OK;
}

// ---- clade sizes of every tree's mutation records (vgx_mutation_spectrum.hip, vgx_mutation_spectrum.h) --------------
// The walk pass of vgx_get_tree_shapes with the host clock left out: the spectrum kernel needs the parents and the mutation records
// alone, so walk and spectrum run on the stream with no host step between them and only the rows, the status pairs, the walk's
// result and the generator words come to the host.
extern "C" int vgx_get_mutation_spectrum(vgx_engine *e, vgx_mutation_spectrum_io *io) {
    if (!e || !io || io->n < 0 ||
        (io->n > 0 && (!io->replicates || !io->rng_state || !io->spectrum || !io->substitutions || !io->sums || !io->stats || !io->status ||
                       !io->status_arg || !io->rng_out)))
        return VGX_ERR_ARG;
    const std::string me = "vgx_get_mutation_spectrum: ";
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
    io->passes = 0;
    io->sites = e->d.sites;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    if (!e->sc_host_valid || !e->dev_state_valid) return fail(e, VGX_ERR_ARG, me + "no direct simulate call yet");
    if (e->last_was_tau) return fail(e, VGX_ERR_ARG, me + "the last call was vgx_simulate_tau (direct chains only)");
    if (!e->call_recorded) return fail(e, VGX_ERR_ARG, me + "the last call did not record events");
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, S = e->d.sites;
    if (S < 0 || S > VGX_MSP_SITES_MAX) return fail(e, VGX_ERR_ARG, me + "the model has " + std::to_string(S) + " sites (0 .. 15)");
    std::vector<int64_t> n_ev((size_t)n), sC((size_t)n);
    {
        std::vector<char> seen((size_t)e->R, 0);
        for (int64_t i = 0; i < n; i++) {
            const int64_t r = io->replicates[i];
            if (r < 0 || r >= e->R) return fail(e, VGX_ERR_ARG, me + "replicate index out of range");
            if (seen[(size_t)r]) return fail(e, VGX_ERR_ARG, me + "replicates must be distinct");
            seen[(size_t)r] = 1;
            const VgxRepScalars &s = e->sc_host[(size_t)r];
            const int64_t first = s.restarts > 0 ? 0 : ((size_t)r < e->call_ev0.size() ? e->call_ev0[(size_t)r] : e->ev_ptr0);
            if (first != 0 || e->ev_base != 0)
                return fail(e, VGX_ERR_ARG, me + "the chain of replicate " + std::to_string(r) +
                                                " does not start in the last call's device log (events.ptr was not 0 at its start)");
            if (s.ev_ptr < 0 || s.ev_ptr > e->evcap || s.ev_ptr >= ((int64_t)1 << 30))
                return fail(e, VGX_ERR_ARG, me + "event range of replicate " + std::to_string(r) + " outside the device log");
            n_ev[(size_t)i] = s.ev_ptr;
            sC[(size_t)i] = s.sCounter;
        }
    }
    if (n == 0) {
        io->ms[2] = since(t_call);
        return VGX_OK;
    }
    HIPCHECK(e, hipSetDevice(e->device));
    const int32_t *log = (const int32_t *)e->r_evcols.p;
    auto up8 = [](int64_t b) { return (b + 255) / 256 * 256; };
    hipError_t er;
    // the MUTATION and MIGRATION events of every chain: the record capacities the walk needs (what the sizing call of vgx_get_genealogies counts)
    std::vector<int64_t> cnt((size_t)n * 2);
    {
        char *cws = nullptr;
        const int64_t o_n = up8(n * 8), o_out = o_n + up8(n * 8);
        if ((er = hipMalloc((void **)&cws, (size_t)(o_out + up8(n * 16)))) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "hipMalloc: " + hipGetErrorString(er));
        std::unique_ptr<char, void (*)(char *)> chold(cws, [](char *p) { (void)hipFree(p); });
        HIPCHECK(e, hipMemcpyAsync(cws, io->replicates, (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(cws + o_n, n_ev.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, vgxi_gw_count(log, e->evcap, (const int64_t *)cws, (const int64_t *)(cws + o_n), n, (int64_t *)(cws + o_out), e->stream));
        HIPCHECK(e, hipMemcpyAsync(cnt.data(), cws + o_out, (size_t)n * 16, hipMemcpyDeviceToHost, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "counting pass: " + hipGetErrorString(er));
    }
    // the walk reads the 8-byte counts of the final occupancy lists
    if (!e->counts64_valid) {
        HIPCHECK(e, vgxi_launch_counts64(e->dr.lcnt32, e->dr.lcnt, e->R * P * e->cap, e->stream));
        HIPCHECK(e, hipStreamSynchronize(e->stream));
        e->counts64_valid = true;
    }
    // per-replicate workspace and outputs (elements), and the passes: every pass holds at most `share` bytes
    const int64_t row_cells = S * (VGX_MSP_BINS + 16 + VGX_MSP_SUMS) + VGX_MSP_STATS + 2;
    std::vector<VgxGwDesc> desc((size_t)n);
    std::vector<int64_t> bytes((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        VgxGwDesc &d = desc[(size_t)i];
        const int64_t nodes = sC[(size_t)i] >= 2 ? 2 * sC[(size_t)i] - 1 : 0;
        d.rep = io->replicates[i];
        d.n_ev = n_ev[(size_t)i];
        d.sCounter = sC[(size_t)i];
        d.tsize = d.sCounter >= 2 ? vgx_gw_table_size(d.n_ev, P * H) : 0;
        d.arena_cap = d.sCounter >= 2 ? d.n_ev : 0;
        d.mut_cap = cnt[(size_t)(2 * i)];
        d.mig_cap = cnt[(size_t)(2 * i + 1)] + nodes;
        for (int k = 0; k < 4; k++) d.rng[k] = io->rng_state[i * 4 + k];
        bytes[(size_t)i] = d.tsize * 28 + d.arena_cap * 4 + nodes * (12 + VGX_MSP_NODE_BYTES) + d.mut_cap * 20 + d.mig_cap * 16 +
                           (int64_t)(sizeof(VgxGwDesc) + sizeof(VgxMspDesc)) + 72 + 8 * row_cells;
    }
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    int64_t share = (int64_t)(free_b / 2);
    if (const char *cb = getenv("VGX_GENEALOGY_CHUNK_BYTES")) share = std::min<int64_t>(share, std::max<int64_t>(atoll(cb), 1));
    struct Events {   // walk and spectrum kernel, timed apart
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
        ~Events() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
    } tm;
    for (hipEvent_t &x : tm.ev) HIPCHECK(e, hipEventCreate(&x));
    int64_t i0 = 0;
    while (i0 < n) {
        int64_t i1 = i0, sum = 0;
        while (i1 < n && (i1 == i0 || sum + bytes[(size_t)i1] <= share)) sum += bytes[(size_t)i1++];
        const int64_t m = i1 - i0;
        int64_t T = 0, A = 0, N = 0, M = 0, G = 0;
        std::vector<VgxGwDesc> dp(desc.begin() + i0, desc.begin() + i1);
        std::vector<VgxMspDesc> md((size_t)m);
        for (int64_t j = 0; j < m; j++) {
            VgxGwDesc &d = dp[(size_t)j];
            const int64_t nodes = d.sCounter >= 2 ? 2 * d.sCounter - 1 : 0;
            d.tab_off = T; d.arena_off = A; d.node_off = N; d.mut_off = M; d.mig_off = G;
            md[(size_t)j] = VgxMspDesc{N, nodes, M, d.mut_cap};
            T += d.tsize; A += d.arena_cap; N += nodes; M += d.mut_cap; G += d.mig_cap;
        }
        // one allocation: the walk's of vgx_get_genealogies [desc | res | rng | key | cnt | base | len | lcap | arena | node x3 | mut x5 | mig x4],
        // then [tree descs | kids, got, n, clade | spectrum | substitutions | sums | stats | status]
        const int64_t o_desc = 0, o_res = o_desc + up8(m * (int64_t)sizeof(VgxGwDesc)), o_rng = o_res + up8(m * 40),
                      o_key = o_rng + up8(m * 32), o_cnt = o_key + up8(T * 8), o_base = o_cnt + up8(T * 8), o_len = o_base + up8(T * 4),
                      o_lcap = o_len + up8(T * 4), o_arena = o_lcap + up8(T * 4), o_out = o_arena + up8(A * 4),
                      o_md = o_out + up8((3 * N + 5 * M + 4 * G) * 4), o_w32 = o_md + up8(m * (int64_t)sizeof(VgxMspDesc)),
                      o_sp = o_w32 + up8(4 * N * 4), o_sub = o_sp + up8(m * S * VGX_MSP_BINS * 8), o_sums = o_sub + up8(m * S * 16 * 8),
                      o_stats = o_sums + up8(m * S * VGX_MSP_SUMS * 8), o_status = o_stats + up8(m * VGX_MSP_STATS * 8), total = o_status + up8(m * 16);
        char *ws = nullptr;
        if ((er = hipMalloc((void **)&ws, (size_t)total)) != hipSuccess)
            return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(total) + " bytes: " + hipGetErrorString(er));
        std::unique_ptr<char, void (*)(char *)> hold(ws, [](char *p) { (void)hipFree(p); });
        VgxGwLaunch a{};
        a.n = m;
        a.desc = (const VgxGwDesc *)(ws + o_desc);
        a.log = log; a.evcap = e->evcap;
        a.nocc = e->dr.nocc; a.lhap = e->dr.lhap; a.lcnt = e->dr.lcnt;
        a.P = P; a.H = H; a.cap = e->cap;
        a.key = (int64_t *)(ws + o_key); a.cnt = (int64_t *)(ws + o_cnt);
        a.base = (int32_t *)(ws + o_base); a.len = (int32_t *)(ws + o_len); a.lcap = (int32_t *)(ws + o_lcap);
        a.arena = (int32_t *)(ws + o_arena);
        int32_t *o32 = (int32_t *)(ws + o_out);
        a.tree = o32; a.tree_pop = o32 + N; a.node_ev = o32 + 2 * N;
        int32_t *mu = o32 + 3 * N;
        a.mut_node = mu; a.mut_AS = mu + M; a.mut_DS = mu + 2 * M; a.mut_site = mu + 3 * M; a.mut_ev = mu + 4 * M;
        int32_t *mg = mu + 5 * M;
        a.mig_node = mg; a.mig_old = mg + G; a.mig_new = mg + 2 * G; a.mig_ev = mg + 3 * G;
        a.res = (int64_t *)(ws + o_res);
        a.rng_out = (uint64_t *)(ws + o_rng);
        VgxMspLaunch b{};
        b.n = m;
        b.desc = (const VgxMspDesc *)(ws + o_md);
        b.res = a.res;
        b.tree = a.tree;
        b.mut_node = a.mut_node; b.mut_AS = a.mut_AS; b.mut_DS = a.mut_DS; b.mut_site = a.mut_site;
        b.S = S;
        int32_t *w32 = (int32_t *)(ws + o_w32);
        b.w = VgxMspWork{w32, w32 + N, w32 + 2 * N, w32 + 3 * N};
        b.spectrum = (int64_t *)(ws + o_sp); b.substitutions = (int64_t *)(ws + o_sub); b.sums = (int64_t *)(ws + o_sums);
        b.stats = (int64_t *)(ws + o_stats); b.status = (int64_t *)(ws + o_status);
        // descriptors up, the walk in wave layout, the spectrum kernel: no host step between them
        HIPCHECK(e, hipMemcpyAsync(ws + o_desc, dp.data(), (size_t)m * sizeof(VgxGwDesc), hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(ws + o_md, md.data(), (size_t)m * sizeof(VgxMspDesc), hipMemcpyHostToDevice, e->stream));
        if (T > 0) HIPCHECK(e, hipMemsetAsync(a.key, 0xFF, (size_t)T * 8, e->stream));   // every slot empty (-1)
        HIPCHECK(e, hipEventRecord(tm.ev[0], e->stream));
        HIPCHECK(e, vgxi_gw_walk(&a, 1, e->stream));
        HIPCHECK(e, hipEventRecord(tm.ev[1], e->stream));
        HIPCHECK(e, vgxi_ms_spectrum(&b, e->stream));
        HIPCHECK(e, hipEventRecord(tm.ev[2], e->stream));
        std::vector<int64_t> st2((size_t)m * 2), res((size_t)m * 5);
        HIPCHECK(e, hipMemcpyAsync(io->spectrum + i0 * S * VGX_MSP_BINS, b.spectrum, (size_t)(m * S * VGX_MSP_BINS) * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->substitutions + i0 * S * 16, b.substitutions, (size_t)(m * S * 16) * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->sums + i0 * S * VGX_MSP_SUMS, b.sums, (size_t)(m * S * VGX_MSP_SUMS) * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->stats + i0 * VGX_MSP_STATS, b.stats, (size_t)m * VGX_MSP_STATS * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(st2.data(), b.status, (size_t)m * 16, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(res.data(), a.res, (size_t)m * 40, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->rng_out + i0 * 4, a.rng_out, (size_t)m * 32, hipMemcpyDeviceToHost, e->stream));
        // the one synchronisation of a pass: before anything reads the rows
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "walk or spectrum kernel failed: " + hipGetErrorString(er));
        float kms = 0.f;
        for (int k = 0; k < 2; k++) {
            HIPCHECK(e, hipEventElapsedTime(&kms, tm.ev[k], tm.ev[k + 1]));
            io->ms[k] += kms;
        }
        for (int64_t j = 0; j < m; j++) {
            // (a walk that stopped keeps its status: the kernel copies it; a walk that used more records than it counted cannot be)
            if (res[(size_t)(j * 5)] == VGX_GW_OK && res[(size_t)(j * 5 + 3)] > dp[(size_t)j].mut_cap)
                return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(dp[(size_t)j].rep) + ": the walk reports more mutation records than its capacity");
            io->status[i0 + j] = st2[(size_t)(2 * j)];
            io->status_arg[i0 + j] = st2[(size_t)(2 * j + 1)];
        }
        io->passes += 1;
        i0 = i1;
    }
    io->ms[2] = since(t_call);
    return VGX_OK;
}

// ---- transmission lineages of every tree (vgx_introductions.hip, vgx_introductions.h) -------------------------------
// The frame of vgx_get_mutation_spectrum: the lineage kernel needs the parents and the node labels alone, so walk and lineages run
// on the stream with no host step between them and only the rows, the status pairs, the walk's result and the generator words
// come to the host.
extern "C" int vgx_get_introductions(vgx_engine *e, vgx_introductions_io *io) {
    if (!e || !io || io->n < 0 ||
        (io->n > 0 && (!io->replicates || !io->rng_state || !io->tips_by_pop || !io->imports || !io->into || !io->spectrum || !io->stats ||
                       !io->status || !io->status_arg || !io->rng_out)))
        return VGX_ERR_ARG;
    const std::string me = "vgx_get_introductions: ";
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
    io->passes = 0;
    io->pops = e->d.popNum;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    if (!e->sc_host_valid || !e->dev_state_valid) return fail(e, VGX_ERR_ARG, me + "no direct simulate call yet");
    if (e->last_was_tau) return fail(e, VGX_ERR_ARG, me + "the last call was vgx_simulate_tau (direct chains only)");
    if (!e->call_recorded) return fail(e, VGX_ERR_ARG, me + "the last call did not record events");
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum;
    if (P < 1 || P > VGX_IN_POPS_MAX)
        return fail(e, VGX_ERR_ARG, me + "the model has " + std::to_string(P) + " populations (1 .. " + std::to_string(VGX_IN_POPS_MAX) + ": a row holds popNum^2 cells)");
    std::vector<int64_t> n_ev((size_t)n), sC((size_t)n);
    {
        std::vector<char> seen((size_t)e->R, 0);
        for (int64_t i = 0; i < n; i++) {
            const int64_t r = io->replicates[i];
            if (r < 0 || r >= e->R) return fail(e, VGX_ERR_ARG, me + "replicate index out of range");
            if (seen[(size_t)r]) return fail(e, VGX_ERR_ARG, me + "replicates must be distinct");
            seen[(size_t)r] = 1;
            const VgxRepScalars &s = e->sc_host[(size_t)r];
            const int64_t first = s.restarts > 0 ? 0 : ((size_t)r < e->call_ev0.size() ? e->call_ev0[(size_t)r] : e->ev_ptr0);
            if (first != 0 || e->ev_base != 0)
                return fail(e, VGX_ERR_ARG, me + "the chain of replicate " + std::to_string(r) +
                                                " does not start in the last call's device log (events.ptr was not 0 at its start)");
            if (s.ev_ptr < 0 || s.ev_ptr > e->evcap || s.ev_ptr >= ((int64_t)1 << 30))
                return fail(e, VGX_ERR_ARG, me + "event range of replicate " + std::to_string(r) + " outside the device log");
            n_ev[(size_t)i] = s.ev_ptr;
            sC[(size_t)i] = s.sCounter;
        }
    }
    if (n == 0) {
        io->ms[2] = since(t_call);
        return VGX_OK;
    }
    HIPCHECK(e, hipSetDevice(e->device));
    const int32_t *log = (const int32_t *)e->r_evcols.p;
    auto up8 = [](int64_t b) { return (b + 255) / 256 * 256; };
    hipError_t er;
    // the MUTATION and MIGRATION events of every chain: the record capacities the walk needs (what the sizing call of vgx_get_genealogies counts)
    std::vector<int64_t> cnt((size_t)n * 2);
    {
        char *cws = nullptr;
        const int64_t o_n = up8(n * 8), o_out = o_n + up8(n * 8);
        if ((er = hipMalloc((void **)&cws, (size_t)(o_out + up8(n * 16)))) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "hipMalloc: " + hipGetErrorString(er));
        std::unique_ptr<char, void (*)(char *)> chold(cws, [](char *p) { (void)hipFree(p); });
        HIPCHECK(e, hipMemcpyAsync(cws, io->replicates, (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(cws + o_n, n_ev.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, vgxi_gw_count(log, e->evcap, (const int64_t *)cws, (const int64_t *)(cws + o_n), n, (int64_t *)(cws + o_out), e->stream));
        HIPCHECK(e, hipMemcpyAsync(cnt.data(), cws + o_out, (size_t)n * 16, hipMemcpyDeviceToHost, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "counting pass: " + hipGetErrorString(er));
    }
    // the walk reads the 8-byte counts of the final occupancy lists
    if (!e->counts64_valid) {
        HIPCHECK(e, vgxi_launch_counts64(e->dr.lcnt32, e->dr.lcnt, e->R * P * e->cap, e->stream));
        HIPCHECK(e, hipStreamSynchronize(e->stream));
        e->counts64_valid = true;
    }
    // per-replicate workspace and outputs (elements), and the passes: every pass holds at most `share` bytes
    const int64_t row_cells = vgx_in_row_cells(P) + 2;
    std::vector<VgxGwDesc> desc((size_t)n);
    std::vector<int64_t> bytes((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        VgxGwDesc &d = desc[(size_t)i];
        const int64_t nodes = sC[(size_t)i] >= 2 ? 2 * sC[(size_t)i] - 1 : 0;
        d.rep = io->replicates[i];
        d.n_ev = n_ev[(size_t)i];
        d.sCounter = sC[(size_t)i];
        d.tsize = d.sCounter >= 2 ? vgx_gw_table_size(d.n_ev, P * H) : 0;
        d.arena_cap = d.sCounter >= 2 ? d.n_ev : 0;
        d.mut_cap = cnt[(size_t)(2 * i)];
        d.mig_cap = cnt[(size_t)(2 * i + 1)] + nodes;
        for (int k = 0; k < 4; k++) d.rng[k] = io->rng_state[i * 4 + k];
        bytes[(size_t)i] = d.tsize * 28 + d.arena_cap * 4 + nodes * (12 + VGX_IN_NODE_BYTES) + d.mut_cap * 20 + d.mig_cap * 16 +
                           (int64_t)(sizeof(VgxGwDesc) + sizeof(VgxInDesc)) + 72 + 8 * row_cells;
    }
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    int64_t share = (int64_t)(free_b / 2);
    if (const char *cb = getenv("VGX_GENEALOGY_CHUNK_BYTES")) share = std::min<int64_t>(share, std::max<int64_t>(atoll(cb), 1));
    struct Events {   // walk and lineage kernel, timed apart
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
        ~Events() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
    } tm;
    for (hipEvent_t &x : tm.ev) HIPCHECK(e, hipEventCreate(&x));
    int64_t i0 = 0;
    while (i0 < n) {
        int64_t i1 = i0, sum = 0;
        while (i1 < n && (i1 == i0 || sum + bytes[(size_t)i1] <= share)) sum += bytes[(size_t)i1++];
        const int64_t m = i1 - i0;
        int64_t T = 0, A = 0, N = 0, M = 0, G = 0;
        std::vector<VgxGwDesc> dp(desc.begin() + i0, desc.begin() + i1);
        std::vector<VgxInDesc> md((size_t)m);
        for (int64_t j = 0; j < m; j++) {
            VgxGwDesc &d = dp[(size_t)j];
            const int64_t nodes = d.sCounter >= 2 ? 2 * d.sCounter - 1 : 0;
            d.tab_off = T; d.arena_off = A; d.node_off = N; d.mut_off = M; d.mig_off = G;
            md[(size_t)j] = VgxInDesc{N, nodes};
            T += d.tsize; A += d.arena_cap; N += nodes; M += d.mut_cap; G += d.mig_cap;
        }
        // one allocation: the walk's of vgx_get_genealogies [desc | res | rng | key | cnt | base | len | lcap | arena | node x3 | mut x5 | mig x4],
        // then [tree descs | kids, got, n, ln | tips_by_pop | imports | into | spectrum | stats | status]
        const int64_t o_desc = 0, o_res = o_desc + up8(m * (int64_t)sizeof(VgxGwDesc)), o_rng = o_res + up8(m * 40),
                      o_key = o_rng + up8(m * 32), o_cnt = o_key + up8(T * 8), o_base = o_cnt + up8(T * 8), o_len = o_base + up8(T * 4),
                      o_lcap = o_len + up8(T * 4), o_arena = o_lcap + up8(T * 4), o_out = o_arena + up8(A * 4),
                      o_md = o_out + up8((3 * N + 5 * M + 4 * G) * 4), o_w32 = o_md + up8(m * (int64_t)sizeof(VgxInDesc)),
                      o_tp = o_w32 + up8(4 * N * 4), o_imp = o_tp + up8(m * P * 8), o_into = o_imp + up8(m * P * P * 8),
                      o_sp = o_into + up8(m * P * VGX_IN_INTO * 8), o_stats = o_sp + up8(m * P * VGX_IN_BINS * 8),
                      o_status = o_stats + up8(m * VGX_IN_STATS * 8), total = o_status + up8(m * 16);
        char *ws = nullptr;
        if ((er = hipMalloc((void **)&ws, (size_t)total)) != hipSuccess)
            return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(total) + " bytes: " + hipGetErrorString(er));
        std::unique_ptr<char, void (*)(char *)> hold(ws, [](char *p) { (void)hipFree(p); });
        VgxGwLaunch a{};
        a.n = m;
        a.desc = (const VgxGwDesc *)(ws + o_desc);
        a.log = log; a.evcap = e->evcap;
        a.nocc = e->dr.nocc; a.lhap = e->dr.lhap; a.lcnt = e->dr.lcnt;
        a.P = P; a.H = H; a.cap = e->cap;
        a.key = (int64_t *)(ws + o_key); a.cnt = (int64_t *)(ws + o_cnt);
        a.base = (int32_t *)(ws + o_base); a.len = (int32_t *)(ws + o_len); a.lcap = (int32_t *)(ws + o_lcap);
        a.arena = (int32_t *)(ws + o_arena);
        int32_t *o32 = (int32_t *)(ws + o_out);
        a.tree = o32; a.tree_pop = o32 + N; a.node_ev = o32 + 2 * N;
        int32_t *mu = o32 + 3 * N;
        a.mut_node = mu; a.mut_AS = mu + M; a.mut_DS = mu + 2 * M; a.mut_site = mu + 3 * M; a.mut_ev = mu + 4 * M;
        int32_t *mg = mu + 5 * M;
        a.mig_node = mg; a.mig_old = mg + G; a.mig_new = mg + 2 * G; a.mig_ev = mg + 3 * G;
        a.res = (int64_t *)(ws + o_res);
        a.rng_out = (uint64_t *)(ws + o_rng);
        VgxInLaunch b{};
        b.n = m;
        b.desc = (const VgxInDesc *)(ws + o_md);
        b.res = a.res;
        b.tree = a.tree; b.pop = a.tree_pop;
        b.P = P;
        int32_t *w32 = (int32_t *)(ws + o_w32);
        b.w = VgxInWork{w32, w32 + N, w32 + 2 * N, w32 + 3 * N};
        b.tips_by_pop = (int64_t *)(ws + o_tp); b.imports = (int64_t *)(ws + o_imp); b.into = (int64_t *)(ws + o_into);
        b.spectrum = (int64_t *)(ws + o_sp); b.stats = (int64_t *)(ws + o_stats); b.status = (int64_t *)(ws + o_status);
        // descriptors up, the rows zeroed (they are counted in place), the walk in wave layout, the lineage kernel: no host step between them
        HIPCHECK(e, hipMemcpyAsync(ws + o_desc, dp.data(), (size_t)m * sizeof(VgxGwDesc), hipMemcpyHostToDevice, e->stream));
        HIPCHECK(e, hipMemcpyAsync(ws + o_md, md.data(), (size_t)m * sizeof(VgxInDesc), hipMemcpyHostToDevice, e->stream));
        if (T > 0) HIPCHECK(e, hipMemsetAsync(a.key, 0xFF, (size_t)T * 8, e->stream));   // every slot empty (-1)
        HIPCHECK(e, hipMemsetAsync(ws + o_tp, 0, (size_t)(o_stats - o_tp), e->stream));
        HIPCHECK(e, hipEventRecord(tm.ev[0], e->stream));
        HIPCHECK(e, vgxi_gw_walk(&a, 1, e->stream));
        HIPCHECK(e, hipEventRecord(tm.ev[1], e->stream));
        HIPCHECK(e, vgxi_in_lineages(&b, e->stream));
        HIPCHECK(e, hipEventRecord(tm.ev[2], e->stream));
        std::vector<int64_t> st2((size_t)m * 2), res((size_t)m * 5);
        HIPCHECK(e, hipMemcpyAsync(io->tips_by_pop + i0 * P, b.tips_by_pop, (size_t)(m * P) * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->imports + i0 * P * P, b.imports, (size_t)(m * P * P) * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->into + i0 * P * VGX_IN_INTO, b.into, (size_t)(m * P * VGX_IN_INTO) * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->spectrum + i0 * P * VGX_IN_BINS, b.spectrum, (size_t)(m * P * VGX_IN_BINS) * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->stats + i0 * VGX_IN_STATS, b.stats, (size_t)m * VGX_IN_STATS * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(st2.data(), b.status, (size_t)m * 16, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(res.data(), a.res, (size_t)m * 40, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(e, hipMemcpyAsync(io->rng_out + i0 * 4, a.rng_out, (size_t)m * 32, hipMemcpyDeviceToHost, e->stream));
        // the one synchronisation of a pass: before anything reads the rows
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "walk or lineage kernel failed: " + hipGetErrorString(er));
        float kms = 0.f;
        for (int k = 0; k < 2; k++) {
            HIPCHECK(e, hipEventElapsedTime(&kms, tm.ev[k], tm.ev[k + 1]));
            io->ms[k] += kms;
        }
        for (int64_t j = 0; j < m; j++) {
            // (a walk that stopped keeps its status: the kernel copies it; a walk that used more nodes than its samples allow cannot be)
            const int64_t nodes = dp[(size_t)j].sCounter >= 2 ? 2 * dp[(size_t)j].sCounter - 1 : 0;
            if (res[(size_t)(j * 5)] == VGX_GW_OK && res[(size_t)(j * 5 + 2)] > nodes)
                return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(dp[(size_t)j].rep) + ": the walk reports more nodes than its samples give");
            io->status[i0 + j] = st2[(size_t)(2 * j)];
            io->status_arg[i0 + j] = st2[(size_t)(2 * j + 1)];
        }
        io->passes += 1;
        i0 = i1;
    }
    io->ms[2] = since(t_call);
    return VGX_OK;
}

// ---- peaks, first passages and last positive events of many replicates (vgx_milestones.hip, vgx_milestones.h) -----
// vgx_get_prevalence's host side with the tile edges in place of a grid: per chunk, pass A (its counting and scan kernels) gives
// every tile its base, the ordered walk merges every tile's records into the block the host initialised from the start state, and
// the host turns the event indices into times with the clock it has just run.
extern "C" int vgx_get_milestones(vgx_engine *e, vgx_milestones_io *io) {
    if (!e || !io || io->n < 0 || (io->n > 0 && !io->replicates)) return VGX_ERR_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    auto wall = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(); };
    io->passes = 0;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    if (e->last_was_tau) return fail(e, VGX_ERR_ARG, "vgx_get_milestones: the last call was vgx_simulate_tau (walks direct chains only)");
    if (!e->sc_host_valid || !e->dev_state_valid) return fail(e, VGX_ERR_ARG, "vgx_get_milestones: needs a direct vgx_simulate_direct call with the event log first");
    if (!e->call_recorded) return fail(e, VGX_ERR_ARG, "vgx_get_milestones: the last call did not record events");
    const int64_t n = io->n, P = e->d.popNum, H = e->d.hapNum, V = io->V, K = io->K;
    if (V < 1 || V > INT32_MAX || !io->variant_of) return fail(e, VGX_ERR_ARG, "vgx_get_milestones: V = " + std::to_string(V) + " classes: at least 1, with variant_of");
    for (int64_t h = 0; h < H; h++)
        if (io->variant_of[h] < -1 || io->variant_of[h] >= V)
            return fail(e, VGX_ERR_ARG, "vgx_get_milestones: variant_of[" + std::to_string(h) + "] = " + std::to_string(io->variant_of[h]) + " is outside [-1, " + std::to_string(V) + ")");
    if (K < 0 || K > VGX_MS_MAX_K || (K > 0 && !io->thresholds))
        return fail(e, VGX_ERR_ARG, "vgx_get_milestones: K = " + std::to_string(K) + " thresholds: at most 16, with thresholds");
    for (int64_t pn = 0; pn < P; pn++)
        if (e->sizes[(size_t)pn] >= ((int64_t)1 << 31)) return fail(e, VGX_ERR_ARG, "vgx_get_milestones: population sizes of 2^31 or more");
    if (vgx_ms_lds_bytes(P, V, K) > VGX_MS_LDS_MAX)
        return fail(e, VGX_ERR_ARG, "vgx_get_milestones: " + std::to_string(P) + " populations (and their total) x " + std::to_string(V) + " classes x " + std::to_string(K) +
                                        " thresholds need " + std::to_string(vgx_ms_lds_bytes(P, V, K)) + " bytes of records, above the " + std::to_string((int64_t)VGX_MS_LDS_MAX) +
                                        " bytes of LDS a walking workgroup may use");
    const int64_t pv = P * V, cells = pv + V;
    std::vector<int32_t> n_ev((size_t)n);
    {
        std::vector<char> seen((size_t)e->R, 0);
        for (int64_t i = 0; i < n; i++) {
            const int64_t r = io->replicates[i];
            if (r < 0 || r >= e->R) return fail(e, VGX_ERR_ARG, "vgx_get_milestones: replicate index out of range");
            if (seen[(size_t)r]) return fail(e, VGX_ERR_ARG, "vgx_get_milestones: replicates must be distinct");
            seen[(size_t)r] = 1;
            const VgxRepScalars &s = e->sc_host[(size_t)r];
            const int64_t first = s.restarts > 0 ? 0 : ((size_t)r < e->call_ev0.size() ? e->call_ev0[(size_t)r] : e->ev_ptr0);
            if (first != 0 || e->ev_base != 0)
                return fail(e, VGX_ERR_ARG, "vgx_get_milestones: replicate " + std::to_string(r) + ": its chain does not start in the last call's device log (the model held " +
                                                std::to_string(e->ev_base != 0 ? e->ev_base : first) + " events when the ensemble started)");
            if (s.ev_ptr >= VGX_MS_MAX_EVENTS)
                return fail(e, VGX_ERR_ARG, "vgx_get_milestones: replicate " + std::to_string(r) + " holds a chain of " + std::to_string(s.ev_ptr) + " events (2^30 or more)");
            if (s.ev_ptr < 0 || s.ev_ptr > e->evcap)
                return fail(e, VGX_ERR_ARG, "vgx_get_milestones: event range of replicate " + std::to_string(r) + " outside the device log");
            n_ev[(size_t)i] = (int32_t)s.ev_ptr;
        }
    }
    if (n == 0) {
        io->ms[2] = wall();
        return VGX_OK;
    }
    // the start of a chain folded through variant_of, the row of all populations behind the population rows
    std::vector<int32_t> start((size_t)(n * pv));
    std::vector<int32_t> start_all[2] = {std::vector<int32_t>((size_t)cells), std::vector<int32_t>((size_t)cells)};
    {
        std::vector<int64_t> fold[2] = {std::vector<int64_t>((size_t)cells, 0), std::vector<int64_t>((size_t)cells, 0)};
        const std::vector<int64_t> *src[2] = {&e->hs.infectious, &e->hs.initial_infectious};
        for (int k = 0; k < 2; k++) {
            for (int64_t pn = 0; pn < P; pn++)
                for (int64_t h = 0; h < H; h++)
                    if (io->variant_of[h] >= 0) {
                        fold[k][(size_t)(pn * V + io->variant_of[h])] += (*src[k])[(size_t)(pn * H + h)];
                        fold[k][(size_t)(pv + io->variant_of[h])] += (*src[k])[(size_t)(pn * H + h)];
                    }
            for (int64_t c = 0; c < cells; c++) {
                if (fold[k][(size_t)c] < 0 || fold[k][(size_t)c] > INT32_MAX) return fail(e, VGX_ERR_ARG, "vgx_get_milestones: a start value outside [0, 2^31)");
                start_all[k][(size_t)c] = (int32_t)fold[k][(size_t)c];
            }
        }
        for (int64_t i = 0; i < n; i++) {
            const std::vector<int32_t> &f = start_all[e->sc_host[(size_t)io->replicates[i]].restarts > 0 ? 1 : 0];
            for (int64_t c = 0; c < pv; c++) start[(size_t)(i * pv + c)] = f[(size_t)c];
        }
    }
    int64_t tile = VGX_MS_TILE_DEFAULT;
    if (const char *tb = getenv("VGX_MILESTONES_TILE_EVENTS")) tile = std::min<int64_t>(std::max<int64_t>(atoll(tb), 1), VGX_MS_MAX_EVENTS);
    const char *wv = getenv("VGX_MILESTONES_WAVES");      // diagnostic: 4 = four wavefronts per tile taking rounds in turn
    const int waves = wv && atoi(wv) == 4 ? 4 : 1;
    HIPCHECK(e, hipSetDevice(e->device));
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    auto up8 = [](int64_t b) { return (b + 255) / 256 * 256; };
    auto dev_free = [](char *p) { (void)hipFree(p); };
    // what stays for the whole call: [rep | n_ev | variant_of | start | peak | last_pos | first]
    const int64_t peak_bytes = n * cells * 8, last_bytes = n * cells * 4, first_bytes = n * K * cells * 4;
    const int64_t o_rep = 0, o_nev = o_rep + up8(n * 8), o_map = o_nev + up8(n * 4), o_start = o_map + up8(H * 4), o_peak = o_start + up8(n * pv * 4),
                  o_last = o_peak + up8(peak_bytes), o_first = o_last + up8(last_bytes), keep_total = o_first + up8(first_bytes) + 256;
    if (keep_total > (int64_t)(free_b / 2))
        return fail(e, VGX_ERR_ARG, "vgx_get_milestones: the block of " + std::to_string(n) + " x " + std::to_string(P + 1) + " x " + std::to_string(V) + " records of " +
                                        std::to_string(K) + " thresholds and its start take " + std::to_string(keep_total) + " bytes, above half of the " +
                                        std::to_string((int64_t)free_b) + " bytes of free device memory: select fewer replicates per call");
    const int64_t share = (int64_t)(free_b / 2) - keep_total + 4096;
    // the bases of one replicate: its bounds, a running sum per (tile, population, class) and the final row
    const int64_t tile_bytes = pv * 4 + 4;
    for (int64_t i = 0; i < n; i++) {
        const int64_t tiles = std::max<int64_t>((n_ev[(size_t)i] + tile - 1) / tile, 1);
        const int64_t need = (int64_t)n_ev[(size_t)i] * 12 + 64 + tiles * tile_bytes + pv * 4 + 1024;
        if (need > share)
            return fail(e, VGX_ERR_ARG, "vgx_get_milestones: replicate " + std::to_string(io->replicates[i]) + ": the bases of its " + std::to_string(tiles) + " tiles of " +
                                            std::to_string(tile) + " events (" + std::to_string(tiles * tile_bytes) + " bytes) and its clock take " + std::to_string(need) +
                                            " bytes, above the " + std::to_string(share) + " bytes of device memory the call may use: raise VGX_MILESTONES_TILE_EVENTS");
    }
    char *kws = nullptr;
    hipError_t er = hipMalloc((void **)&kws, (size_t)keep_total);
    if (er != hipSuccess) return fail(e, VGX_ERR_HIP, "vgx_get_milestones: hipMalloc of " + std::to_string(keep_total) + " bytes: " + hipGetErrorString(er));
    std::unique_ptr<char, void (*)(char *)> khold(kws, dev_free);
    std::vector<int64_t> reps_all(io->replicates, io->replicates + n);
    // the block before any tile: the start offers itself at event -1
    std::vector<uint64_t> h_peak((size_t)(n * cells));
    std::vector<int32_t> h_last((size_t)(n * cells)), h_first((size_t)(n * std::max<int64_t>(K, 1) * cells));
    for (int64_t i = 0; i < n; i++) {
        const std::vector<int32_t> &f = start_all[e->sc_host[(size_t)io->replicates[i]].restarts > 0 ? 1 : 0];
        const VgxMsBlock b{h_peak.data() + i * cells, h_last.data() + i * cells, h_first.data() + i * K * cells};
        for (int64_t c = 0; c < cells; c++) vgx_ms_init_cell(b, (int32_t)c, (int32_t)cells, f[(size_t)c], io->thresholds, (int32_t)K);
    }
    HIPCHECK(e, hipMemcpyAsync(kws + o_rep, reps_all.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_nev, n_ev.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_map, io->variant_of, (size_t)H * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_start, start.data(), (size_t)(n * pv) * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_peak, h_peak.data(), (size_t)peak_bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_last, h_last.data(), (size_t)last_bytes, hipMemcpyHostToDevice, e->stream));
    if (K > 0) HIPCHECK(e, hipMemcpyAsync(kws + o_first, h_first.data(), (size_t)first_bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipStreamSynchronize(e->stream));

    std::vector<std::vector<double>> tms((size_t)n);      // the event times of the chunk's replicates, until their indices are known
    const int rc_chunks = clock_chunks(e, "vgx_get_milestones", reps_all, n_ev, (const int64_t *)(kws + o_rep), (const int32_t *)(kws + o_nev), share, io->ms,
        // host: a replicate's event times are kept until the chunk's event indices come back
        [&](int64_t gi, const std::vector<double> &times) { tms[(size_t)gi] = times; },
        // device: pass A over the tile edges, then the walk of every (replicate, tile); host: indices -> results and times
        [&](int64_t i0, int64_t i1, int64_t max_n) -> int {
            const int64_t m = i1 - i0, T = std::max<int64_t>((max_n + tile - 1) / tile, 1);
            std::vector<int32_t> bounds((size_t)(m * (T + 2)));
            for (int64_t j = 0; j < m; j++)
                for (int64_t k = 0; k <= T + 1; k++) bounds[(size_t)(j * (T + 2) + k)] = (int32_t)std::min<int64_t>(k * tile, n_ev[(size_t)(i0 + j)]);
            const int64_t c_bnd = 0, c_val = c_bnd + up8(m * (T + 2) * 4), c_fin = c_val + up8(m * T * pv * 4), c_total = c_fin + up8(m * pv * 4);
            char *cws = nullptr;
            if ((er = hipMalloc((void **)&cws, (size_t)c_total)) != hipSuccess)
                return fail(e, VGX_ERR_HIP, "vgx_get_milestones: hipMalloc of " + std::to_string(c_total) + " bytes: " + hipGetErrorString(er));
            std::unique_ptr<char, void (*)(char *)> chold(cws, dev_free);
            HIPCHECK(e, hipMemcpyAsync(cws + c_bnd, bounds.data(), bounds.size() * 4, hipMemcpyHostToDevice, e->stream));
            HIPCHECK(e, hipMemsetAsync(cws + c_val, 0, (size_t)(c_total - c_val), e->stream));   // val and fin
            HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
            VgxMsLaunch g{};
            VgxPrevLaunch &a = g.a;
            a.m = m;
            a.log = (const int32_t *)e->r_evcols.p; a.evcap = e->evcap;
            a.rep = (const int64_t *)(kws + o_rep) + i0; a.n_ev = (const int32_t *)(kws + o_nev) + i0;
            a.bound = (const int32_t *)(cws + c_bnd);
            a.T = (int32_t)T; a.P = (int32_t)P; a.hapNum = (int32_t)H; a.V = (int32_t)V;
            a.variant_of = (const int32_t *)(kws + o_map);
            a.tile = (int32_t)tile; a.max_n = max_n;
            a.val = (int32_t *)(cws + c_val);
            a.fin = (int32_t *)(cws + c_fin);
            a.start = (const int32_t *)(kws + o_start) + i0 * pv;
            g.K = (int32_t)K;
            for (int64_t k = 0; k < K; k++) g.theta[k] = io->thresholds[k];
            g.peak = (uint64_t *)(kws + o_peak) + i0 * cells;
            g.last_pos = (int32_t *)(kws + o_last) + i0 * cells;
            g.first = (int32_t *)(kws + o_first) + i0 * K * cells;
            HIPCHECK(e, vgxi_prev_count(&a, e->stream));
            HIPCHECK(e, vgxi_prev_scan(&a, e->stream));
            HIPCHECK(e, vgxi_ms_walk(&g, waves, e->stream));
            if (max_n > 0) io->passes += 1;
            HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
            std::vector<int32_t> fin((size_t)(m * pv));
            HIPCHECK(e, hipMemcpyAsync(fin.data(), cws + c_fin, (size_t)(m * pv) * 4, hipMemcpyDeviceToHost, e->stream));
            HIPCHECK(e, hipMemcpyAsync(h_peak.data() + i0 * cells, kws + o_peak + i0 * cells * 8, (size_t)(m * cells) * 8, hipMemcpyDeviceToHost, e->stream));
            HIPCHECK(e, hipMemcpyAsync(h_last.data() + i0 * cells, kws + o_last + i0 * cells * 4, (size_t)(m * cells) * 4, hipMemcpyDeviceToHost, e->stream));
            if (K > 0)
                HIPCHECK(e, hipMemcpyAsync(h_first.data() + i0 * K * cells, kws + o_first + i0 * K * cells * 4, (size_t)(m * K * cells) * 4, hipMemcpyDeviceToHost, e->stream));
            if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)
                return fail(e, VGX_ERR_HIP, std::string("vgx_get_milestones: counting, scan or walk kernel failed: ") + hipGetErrorString(er));
            float kms = 0.f;
            HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
            io->ms[0] += kms;
            for (int64_t j = 0; j < m; j++) {
                const int64_t gi = i0 + j, r = reps_all[(size_t)gi];
                const VgxMsBlock b{h_peak.data() + gi * cells, h_last.data() + gi * cells, h_first.data() + gi * K * cells};
                auto at = [&](auto *p, int64_t per) { return p ? p + gi * per : p; };
                const VgxMsOut out{at(io->final, cells), at(io->peak, cells), at(io->peak_event, cells), at(io->last_positive_event, cells),
                                   at(io->first_event, K * cells), at(io->peak_time, cells), at(io->extinction_time, cells), at(io->first_time, K * cells)};
                // index -1: what the host clock opens this chain's run with (clock_build)
                const double t_start = e->sc_host[(size_t)r].restarts > 0 ? 0.0 : e->call_t0[(size_t)r];
                vgx_ms_outputs(b, fin.data() + j * pv, (int32_t)P, (int32_t)V, (int32_t)K, n_ev[(size_t)gi], tms[(size_t)gi].data(), t_start, out);
                std::vector<double>().swap(tms[(size_t)gi]);
            }
            return VGX_OK;
        }, tile, tile_bytes);
    if (rc_chunks) return rc_chunks;
    io->ms[2] = wall();
    return VGX_OK;
}

// ---- susceptible hosts per class of immunity groups of many replicates at the times of one grid (vgx_susceptible.hip,
// vgx_susceptible.h).  vgx_get_prevalence over the other half of the state: the same host clock, bounds, net block,
// scan, min/max pass and summary, with the counting kernel of the susceptible rule and the susceptible start state.
extern "C" int vgx_get_susceptibles(vgx_engine *e, vgx_susceptibles_io *io) {
    if (!e || !io || io->n < 0 || (io->n > 0 && (!io->replicates || !io->outside))) return VGX_ERR_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    auto wall = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(); };
    const std::string me = "vgx_get_susceptibles: ";
    io->passes = 0;
    io->ms[0] = io->ms[1] = io->ms[2] = 0.0;
    if (e->last_was_tau) return fail(e, VGX_ERR_ARG, me + "the last call was vgx_simulate_tau (counts direct chains only)");
    if (!e->sc_host_valid || !e->dev_state_valid) return fail(e, VGX_ERR_ARG, me + "needs a direct vgx_simulate_direct call with the event log first");
    if (!e->call_recorded) return fail(e, VGX_ERR_ARG, me + "the last call did not record events");
    const int64_t n = io->n, P = e->d.popNum, S = e->d.susNum, T = io->T, G = io->G;
    if (T < 1 || T >= VGX_PREV_MAX_POINTS || !io->grid) return fail(e, VGX_ERR_ARG, me + "T = " + std::to_string(T) + " grid points: at least 1, below 2^24, with grid");
    for (int64_t k = 0; k < T; k++) {
        if (!std::isfinite(io->grid[k])) return fail(e, VGX_ERR_ARG, me + "grid[" + std::to_string(k) + "] is not finite");
        if (k > 0 && !(io->grid[k - 1] < io->grid[k])) return fail(e, VGX_ERR_ARG, me + "grid must increase strictly (grid[" + std::to_string(k) + "])");
    }
    if (G < 1 || G > INT32_MAX || !io->class_of) return fail(e, VGX_ERR_ARG, me + "G = " + std::to_string(G) + " classes: at least 1, with class_of");
    for (int64_t g = 0; g < S; g++)
        if (io->class_of[g] < -1 || io->class_of[g] >= G)
            return fail(e, VGX_ERR_ARG, me + "class_of[" + std::to_string(g) + "] = " + std::to_string(io->class_of[g]) + " is outside [-1, " + std::to_string(G) + ")");
    for (int64_t pn = 0; pn < P; pn++)
        if (e->sizes[(size_t)pn] >= ((int64_t)1 << 31)) return fail(e, VGX_ERR_ARG, me + "population sizes of 2^31 or more");
    if (vgx_prev_lds_bytes(P, G) > VGX_PREV_LDS_MAX)
        return fail(e, VGX_ERR_ARG, me + std::to_string(P) + " populations x " + std::to_string(G) + " classes need " + std::to_string(vgx_prev_lds_bytes(P, G)) +
                                        " bytes of cells, above the " + std::to_string((int64_t)VGX_PREV_LDS_MAX) + " bytes of LDS a counting workgroup may use");
    const int64_t cells = P * G;
    std::vector<int32_t> n_ev((size_t)n);
    {
        std::vector<char> seen((size_t)e->R, 0);
        for (int64_t i = 0; i < n; i++) {
            const int64_t r = io->replicates[i];
            if (r < 0 || r >= e->R) return fail(e, VGX_ERR_ARG, me + "replicate index out of range");
            if (seen[(size_t)r]) return fail(e, VGX_ERR_ARG, me + "replicates must be distinct");
            seen[(size_t)r] = 1;
            const VgxRepScalars &s = e->sc_host[(size_t)r];
            const int64_t first = s.restarts > 0 ? 0 : ((size_t)r < e->call_ev0.size() ? e->call_ev0[(size_t)r] : e->ev_ptr0);
            if (first != 0 || e->ev_base != 0)
                return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + ": its chain does not start in the last call's device log (the model held " +
                                                std::to_string(e->ev_base != 0 ? e->ev_base : first) + " events when the ensemble started)");
            if (s.ev_ptr >= VGX_PREV_MAX_EVENTS)
                return fail(e, VGX_ERR_ARG, me + "replicate " + std::to_string(r) + " holds a chain of " + std::to_string(s.ev_ptr) + " events (2^30 or more)");
            if (s.ev_ptr < 0 || s.ev_ptr > e->evcap) return fail(e, VGX_ERR_ARG, me + "event range of replicate " + std::to_string(r) + " outside the device log");
            n_ev[(size_t)i] = (int32_t)s.ev_ptr;
        }
    }
    if (n == 0) {
        io->ms[2] = wall();
        return VGX_OK;
    }
    // the start of a chain folded through class_of: the state the call started from, or the initial state after a restart
    std::vector<int32_t> start((size_t)(n * cells));
    {
        std::vector<int64_t> fold[2] = {std::vector<int64_t>((size_t)cells, 0), std::vector<int64_t>((size_t)cells, 0)};
        const std::vector<int64_t> *src[2] = {&e->hs.susceptible, &e->hs.initial_susceptible};
        for (int k = 0; k < 2; k++)
            for (int64_t pn = 0; pn < P; pn++)
                for (int64_t g = 0; g < S; g++)
                    if (io->class_of[g] >= 0) fold[k][(size_t)(pn * G + io->class_of[g])] += (*src[k])[(size_t)(pn * S + g)];
        for (int k = 0; k < 2; k++)
            for (int64_t c = 0; c < cells; c++)
                if (fold[k][(size_t)c] < 0 || fold[k][(size_t)c] > INT32_MAX) return fail(e, VGX_ERR_ARG, me + "a start value outside [0, 2^31)");
        for (int64_t i = 0; i < n; i++) {
            const std::vector<int64_t> &f = fold[e->sc_host[(size_t)io->replicates[i]].restarts > 0 ? 1 : 0];
            for (int64_t c = 0; c < cells; c++) start[(size_t)(i * cells + c)] = (int32_t)f[(size_t)c];
        }
    }
    int64_t tile = VGX_PREV_TILE_DEFAULT;
    if (const char *tb = getenv("VGX_PREVALENCE_TILE_EVENTS")) tile = std::min<int64_t>(std::max<int64_t>(atoll(tb), 1), VGX_PREV_MAX_EVENTS);
    HIPCHECK(e, hipSetDevice(e->device));
    size_t free_b = 0, total_b = 0;
    HIPCHECK(e, hipMemGetInfo(&free_b, &total_b));
    auto up8 = [](int64_t b) { return (b + 255) / 256 * 256; };
    auto dev_free = [](char *p) { (void)hipFree(p); };
    // what stays for the whole call: [rep | n_ev | bound | class_of | start | val | fin | min, max]
    const int64_t val_bytes = n * T * cells * 4, fin_bytes = n * cells * 4;
    const int64_t o_rep = 0, o_nev = o_rep + up8(n * 8), o_bnd = o_nev + up8(n * 4), o_map = o_bnd + up8(n * (T + 2) * 4), o_start = o_map + up8(S * 4),
                  o_val = o_start + up8(fin_bytes), o_fin = o_val + up8(val_bytes), o_mm = o_fin + up8(fin_bytes), keep_total = o_mm + 256;
    if (keep_total > (int64_t)(free_b / 2))
        return fail(e, VGX_ERR_ARG, me + "the block of " + std::to_string(n) + " x " + std::to_string(T + 1) + " x " + std::to_string(P) + " x " + std::to_string(G) +
                                        " values (" + std::to_string(val_bytes + fin_bytes) + " bytes), its cuts and start take " + std::to_string(keep_total) +
                                        " bytes, above half of the " + std::to_string((int64_t)free_b) + " bytes of free device memory: select fewer replicates per call");
    char *kws = nullptr;
    hipError_t er = hipMalloc((void **)&kws, (size_t)keep_total);
    if (er != hipSuccess) return fail(e, VGX_ERR_HIP, me + "hipMalloc of " + std::to_string(keep_total) + " bytes: " + hipGetErrorString(er));
    std::unique_ptr<char, void (*)(char *)> khold(kws, dev_free);
    std::vector<int64_t> reps_all(io->replicates, io->replicates + n);
    HIPCHECK(e, hipMemcpyAsync(kws + o_rep, reps_all.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_nev, n_ev.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_map, io->class_of, (size_t)S * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemcpyAsync(kws + o_start, start.data(), (size_t)fin_bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(e, hipMemsetAsync(kws + o_val, 0, (size_t)(o_mm - o_val), e->stream));   // val and fin, zeroed once

    const int64_t share = (int64_t)(free_b / 2) - keep_total + 4096;
    std::vector<int32_t> bounds((size_t)(n * (T + 2)));
    const int rc_chunks = clock_chunks(e, "vgx_get_susceptibles", reps_all, n_ev, (const int64_t *)(kws + o_rep), (const int32_t *)(kws + o_nev), share, io->ms,
        // host: a replicate's event times -> its T + 2 bounds
        [&](int64_t gi, const std::vector<double> &times) {
            int32_t *bound = bounds.data() + gi * (T + 2);
            VgxPrevCutter ct{io->grid, T, bound};
            for (size_t k = 0; k < times.size(); k++) ct.event((int64_t)k, times[k]);
            ct.finish((int64_t)times.size());
            io->outside[2 * gi] = bound[1];
            io->outside[2 * gi + 1] = (int64_t)times.size() - bound[(size_t)T];
        },
        // device: the net changes of the chunk's replicates into their rows of the block, then the running sums of those rows
        [&](int64_t i0, int64_t i1, int64_t max_n) -> int {
            const int64_t m = i1 - i0;
            HIPCHECK(e, hipMemcpyAsync(kws + o_bnd + i0 * (T + 2) * 4, bounds.data() + i0 * (T + 2), (size_t)(m * (T + 2)) * 4, hipMemcpyHostToDevice, e->stream));
            HIPCHECK(e, hipEventRecord(e->ev0, e->stream));
            VgxPrevLaunch a{};
            a.m = m;
            a.log = (const int32_t *)e->r_evcols.p; a.evcap = e->evcap;
            a.rep = (const int64_t *)(kws + o_rep) + i0; a.n_ev = (const int32_t *)(kws + o_nev) + i0;
            a.bound = (const int32_t *)(kws + o_bnd) + i0 * (T + 2);
            a.T = (int32_t)T; a.P = (int32_t)P; a.hapNum = (int32_t)S; a.V = (int32_t)G;   // the launch of §18 with susNum, G and class_of
            a.variant_of = (const int32_t *)(kws + o_map);
            a.tile = (int32_t)tile; a.max_n = max_n;
            a.val = (int32_t *)(kws + o_val) + i0 * T * cells;
            a.fin = (int32_t *)(kws + o_fin) + i0 * cells;
            a.start = (const int32_t *)(kws + o_start) + i0 * cells;
            HIPCHECK(e, vgxi_sus_count(&a, e->stream));
            if (max_n > 0) io->passes += 1;
            HIPCHECK(e, vgxi_prev_scan(&a, e->stream));
            HIPCHECK(e, hipEventRecord(e->ev1, e->stream));
            if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "counting or scan kernel failed: " + hipGetErrorString(er));
            float kms = 0.f;
            HIPCHECK(e, hipEventElapsedTime(&kms, e->ev0, e->ev1));
            io->ms[0] += kms;
            return VGX_OK;
        });
    if (rc_chunks) return rc_chunks;
    if (io->values) HIPCHECK(e, hipMemcpy(io->values, kws + o_val, (size_t)val_bytes, hipMemcpyDeviceToHost));
    if (io->final) HIPCHECK(e, hipMemcpy(io->final, kws + o_fin, (size_t)fin_bytes, hipMemcpyDeviceToHost));
    if (io->summary) {
        // the column summary sorts 32-bit keys of whole numbers in [0, 2^31)
        int32_t mm[2] = {0, 0};
        HIPCHECK(e, vgxi_prev_minmax((const int32_t *)(kws + o_val), n * T * cells, (int32_t *)(kws + o_mm), e->stream));
        HIPCHECK(e, hipMemcpyAsync(mm, kws + o_mm, sizeof mm, hipMemcpyDeviceToHost, e->stream));
        if ((er = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(e, VGX_ERR_HIP, me + "min/max kernel failed: " + hipGetErrorString(er));
        if (mm[0] < 0)
            return fail(e, VGX_ERR_ARG, me + "summary: a value of " + std::to_string(mm[0]) + " is not a whole number in [0, 2^31) (the log holds records outside the model)");
        char msg[512] = "";
        const int rc = vgxi_column_summary_i32("vgx_get_susceptibles: summary", (const int32_t *)(kws + o_val), n, T * cells, io->summary, e->stream, msg, sizeof msg);
        if (rc) return fail(e, rc, msg);
    }
    io->ms[2] = wall();
    return VGX_OK;
}
