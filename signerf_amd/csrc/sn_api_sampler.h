// sn_api_sampler.h (part of sn_api.hip) -- include/signerf_hip_sampler.h: training-mode proposal sampling, one wave per ray
#pragma once

static_assert(SN_SAMPLER_MAX_SAMPLES == SN_SAMPLER_MAX_S, "the header's sample limit is the kernels'");
static_assert(SN_SAMPLER_MAX_S == SN_LOSS_MAX_S, "the samplers feed the loss kernels: one limit");

namespace {

// The checks both entry points share, in this order, and the parameter block filled from the rays struct; *launch says whether anything
// is left to do.  Nothing here touches the device.
int check_sampler(const std::string& who, const SnSamplerRays* rays_in, SnSamplerRays& rays, SnSamplerParams& p, bool* launch) {
    *launch = false;
    if (!rays_in) return fail(nullptr, SN_ERR_INVALID, who + ": NULL argument (rays)");
    if (int rc = adopt_struct(nullptr, rays_in, sizeof(SnSamplerRays), rays, (who + ": SnSamplerRays").c_str())) return rc;
    if (rays.n_rays < 0) return fail(nullptr, SN_ERR_INVALID, who + ": n_rays must be >= 0");
    if (rays.n_samples < 1 || rays.n_samples > SN_SAMPLER_MAX_S)
        return fail(nullptr, SN_ERR_INVALID, who + ": n_samples must lie in 1.." + std::to_string(SN_SAMPLER_MAX_S));
    if (rays.spacing_mode != 0 && rays.spacing_mode != 1) return fail(nullptr, SN_ERR_INVALID, who + ": spacing_mode must be 0 (piecewise) or 1 (uniform)");
    memset(&p, 0, sizeof(p));
    p.origins = rays.origins;
    p.directions = rays.directions;
    p.nears = rays.nears;
    p.fars = rays.fars;
    p.near_plane = rays.near_plane;
    p.far_plane = rays.far_plane;
    p.spacing_uniform = rays.spacing_mode;
    p.single_jitter = rays.single_jitter ? 1 : 0;
    p.rand = rays.rand;
    p.seed = rays.seed;
    p.offset = rays.offset;
    p.M = rays.n_samples;
    p.spacing_bins = rays.spacing_bins;
    p.euclid_bins = rays.euclid_bins;
    p.deltas = rays.deltas;
    p.positions = rays.positions;
    p.q = rays.q;
    p.selector = rays.selector;
    p.rand_out = rays.rand_out;
    *launch = true;
    return SN_OK;
}

// the checks behind the entry point's own: R == 0 is SN_OK with nothing launched (an empty tensor's pointer may be NULL)
int launch_sampler(const std::string& who, const SnSamplerRays& rays, bool pointers_ok, const char* pointers, void (*kernel)(SnSamplerParams),
                   size_t lds_bytes, const SnSamplerParams& p, SnStream stream) {
    if (rays.n_rays == 0) return SN_OK;
    if (!pointers_ok) return fail(nullptr, SN_ERR_INVALID, who + ": NULL argument (" + pointers + ")");
    if (rays.n_rays > 0x7fffffffll) return fail(nullptr, SN_ERR_INVALID, who + ": n_rays exceeds the grid (2^31 - 1 rays)");
    hipLaunchKernelGGL(kernel, dim3((unsigned)rays.n_rays), dim3(64), lds_bytes, (hipStream_t)stream, p);
    return end_launches(who);
}

}  // namespace

extern "C" {

int sn_sampler_abi_version(void) { return SN_SAMPLER_ABI_VERSION; }

int sn_sampler_initial(const SnSamplerRays* rays_in, const float* base_bins, SnStream stream) {
    const std::string who = "sn_sampler_initial";
    SnSamplerRays rays;
    SnSamplerParams p;
    bool launch;
    if (int rc = check_sampler(who, rays_in, rays, p, &launch)) return rc;
    p.grid = base_bins;
    return launch_sampler(who, rays, rays.origins && rays.directions && base_bins, "origins, directions, base_bins", sn_train_sampler_initial_kernel,
                          sn_sampler_lds_initial(p.M), p, stream);
}

int sn_sampler_pdf(const SnSamplerRays* rays_in, const SnSamplerPdf* pdf_in, SnStream stream) {
    const std::string who = "sn_sampler_pdf";
    SnSamplerRays rays;
    SnSamplerPdf pdf;
    SnSamplerParams p;
    bool launch;
    if (int rc = check_sampler(who, rays_in, rays, p, &launch)) return rc;
    if (!pdf_in) return fail(nullptr, SN_ERR_INVALID, who + ": NULL argument (pdf)");
    if (int rc = adopt_struct(nullptr, pdf_in, sizeof(SnSamplerPdf), pdf, (who + ": SnSamplerPdf").c_str())) return rc;
    if (pdf.n_in < 1 || pdf.n_in > SN_SAMPLER_MAX_S) return fail(nullptr, SN_ERR_INVALID, who + ": n_in must lie in 1.." + std::to_string(SN_SAMPLER_MAX_S));
    if (!(pdf.anneal >= 0.0f) || !std::isfinite(pdf.anneal)) return fail(nullptr, SN_ERR_INVALID, who + ": anneal must be finite and >= 0");
    if (!std::isfinite(pdf.histogram_padding)) return fail(nullptr, SN_ERR_INVALID, who + ": histogram_padding must be finite");
    p.grid = pdf.u_grid;
    p.sbins = pdf.spacing_bins;
    p.weights = pdf.weights;
    p.N = pdf.n_in;
    p.anneal = pdf.anneal;
    p.hist_pad = pdf.histogram_padding;
    return launch_sampler(who, rays, rays.origins && rays.directions && pdf.spacing_bins && pdf.weights && pdf.u_grid,
                          "origins, directions, spacing_bins, weights, u_grid", sn_train_sampler_pdf_kernel, sn_sampler_lds_pdf(p.N, p.M), p, stream);
}

}  // extern "C"
