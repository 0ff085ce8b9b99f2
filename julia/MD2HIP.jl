# MD2HIP.jl -- the Julia host binding of libmd2hip.so (include/md2.h) for Monodepth2.jl.
#
# Drop-in for the reference's GPU hot path: `include("MD2HIP.jl")` from src/Monodepth.jl (after
# `using AMDGPU, ChainRulesCore`), then use MD2HIP.HIPModel / MD2HIP.train_loss where the reference
# uses Model / train_loss (src/training.jl:21-78, scripts/script.jl:84-86).  Every op below is a
# forward `ccall` plus a `ChainRulesCore.rrule` whose pullback is the library's hand-written HIP
# pullback -- the reference's own plugin mechanism (src/utils.jl:134-145, src/repeat.jl:44-69).
#
# Julia is not installed in the build container: this file is the binding a maintainer adds; the
# Python mirror monodepth2.jl_amd/md2hip/ makes the same calls and is what the tests execute.
#
# Layout contract (INTEGRATION.md): Julia column-major (W,H,C,N) arrays have the bytes of the
# library's C-order [n][c][h][w]; 3x3 matrices go row-major (`vec(permutedims(K))`); Flux Conv
# weights (kw,kh,cin,cout) are true convolutions -> flipped once into the library's
# cross-correlation layout by `flat_params`.
module MD2HIP

using AMDGPU
using ChainRulesCore
import Flux

const lib = get(ENV, "MD2HIP_LIB",
                joinpath(@__DIR__, "..", "monodepth2.jl_amd", "lib", "libmd2hip.so"))

const ABI_VERSION = 2                                  # include/md2.h MD2_ABI_VERSION
function __init__()
    v = ccall((:md2_abi_version, lib), Cint, ())
    v == ABI_VERSION || error("libmd2hip at ", lib, " has ABI version ", v,
                              ", MD2HIP.jl expects ", ABI_VERSION, ": rebuild or update the binding")
end

check(rc) = rc == 0 || error("libmd2hip (", rc, "): ",
                             unsafe_string(ccall((:md2_last_error, lib), Cstring, ())))
stream_ptr() = AMDGPU.stream().stream                  # hipStream_t of the task-local stream
rowmajor(M) = ntuple(i -> Float32(M[(i - 1) ÷ 3 + 1, (i - 1) % 3 + 1]), 9)
pad5(v, T) = ntuple(i -> i <= length(v) ? T(v[i]) : zero(T), 5)
ptr(a) = a === nothing ? C_NULL : pointer(a)

# ------------------------------------------------------------------------------------------------
# C structs (field order and types exactly as include/md2.h)
# ------------------------------------------------------------------------------------------------
struct ModelCfg                                        # md2_model_cfg
    arch::Cint; in_channels::Cint; batch::Cint; width::Cint; height::Cint
    n_levels::Cint; scale_levels::NTuple{5,Cint}
    K::NTuple{9,Cfloat}; invK::NTuple{9,Cfloat}
    min_depth::Cfloat; max_depth::Cfloat; disparity_smoothness::Cfloat
    scales::NTuple{5,Cfloat}; automasking::Cint
    target::Cint; src0::Cint; src1::Cint
    embedding_levels::Cint; num_bins::Cint
end

# Params / TrainCache of src/Monodepth.jl:37-60 -> md2_model_cfg.  MPI mode (src/model.jl:1-55):
# embedding_levels = 21 (DepthDecoder(; embedding_levels)) and num_bins disparity planes, batch 1
function ModelCfg(arch, in_ch, scale_levels, p, c; embedding_levels=0, num_bins=1)
    ModelCfg(arch, in_ch, p.batch_size, p.target_size..., length(scale_levels),
             pad5(scale_levels, Cint), rowmajor(c.K), rowmajor(c.invK),
             p.min_depth, p.max_depth, p.disparity_smoothness, pad5(c.scales, Cfloat),
             p.automasking, c.target_id - 1, c.source_ids[1] - 1, c.source_ids[2] - 1,
             embedding_levels, num_bins)
end

struct LossCfg                                         # md2_loss_cfg
    n::Cint; c::Cint; width::Cint; height::Cint; nscales::Cint
    scale_w::NTuple{5,Cint}; scale_h::NTuple{5,Cint}
    smooth_weight::NTuple{5,Cfloat}; divisor::Cfloat; smooth_normalize::Cint
    K::NTuple{9,Cfloat}; invK::NTuple{9,Cfloat}
    min_depth::Cfloat; max_depth::Cfloat
    x_sample_stride::Clonglong; x_frame_stride::Clonglong
    target::Cint; src0::Cint; src1::Cint; invert_mask::Cint; sigmoid_grad::Cint
end

struct LossOut                                         # md2_loss_out
    loss::Ptr{Float32}; terms::Ptr{Float32}
    d_disp::NTuple{5,Ptr{Float32}}; d_pose::Ptr{Float32}
    vis_loss::Ptr{Float32}; vis_sel::Ptr{Int8}; vis_warped::Ptr{Float32}
    vis_cell::Ptr{Int32}                               # parity diagnostics (not used here)
end

const MAX_SOURCES = 3                                  # include/md2.h MD2_MAX_SOURCES
struct LossSource                                      # md2_loss_source
    frames::Ptr{Float32}; sample_stride::Clonglong
    pose_block::Cint; invert::Cint
    Rt::Ptr{Float32}
end

struct WarpCfg                                         # md2_warp_cfg
    n::Cint; c::Cint; width::Cint; height::Cint; dw::Cint; dh::Cint
    K::NTuple{9,Cfloat}; invK::NTuple{9,Cfloat}
    min_depth::Cfloat; max_depth::Cfloat
    x_sample_stride::Clonglong; x_frame_stride::Clonglong
    target::Cint; src0::Cint; src1::Cint
end

struct ConvDesc                                        # md2_conv_desc
    n::Cint; cin::Cint; h::Cint; w::Cint; cout::Cint; kh::Cint; kw::Cint
    stride::Cint; pad::Cint; reflect::Cint; act::Cint
end

struct DepthEvalCfg                                    # md2_depth_eval_cfg
    n::Cint; h::Cint; w::Cint
    gt_h::Cint; gt_w::Cint
    y0::Cint; y1::Cint; x0::Cint; x1::Cint
    min_depth::Cfloat; max_depth::Cfloat
    eval_min::Cfloat; eval_max::Cfloat
    median_scaling::Cint
    scale::Cfloat
end

struct LidarCfg                                        # md2_lidar_cfg
    n::Cint; h::Cint; w::Cint
    forward_only::Cint
    vel_depth::Cint
end

struct ResizeCfg                                       # md2_resize_cfg
    m::Cint; c::Cint
    out_h::Cint; out_w::Cint
    filter::Cint
    quantize::Cint
end

struct Jitter                                          # md2_jitter
    brightness::Cfloat; contrast::Cfloat; saturation::Cfloat; hue::Cfloat
    order::NTuple{4, Cuchar}
    apply::Cint
end

# ------------------------------------------------------------------------------------------------
# The model: Model(ResidualNetwork, DepthDecoder, PoseDecoder) with its parameters in ONE flat
# device vector (Flux `params(model)` order, md2_arch_param_info) -- src/model.jl:24-70
# ------------------------------------------------------------------------------------------------
mutable struct HIPModel
    handle::Ptr{Cvoid}
    cfg::ModelCfg
    θ::ROCVector{Float32}          # the trainable parameters, library layout (conv taps as
                                   # cross-correlation); Flux.params(m) == Params([m.θ])
    ∇θ::ROCVector{Float32}         # the library's gradient buffer (same layout)
    m::ROCVector{Float32}; v::ROCVector{Float32}; step::Int   # library ADAM state (update!)
    packed::Bool                   # the library's packed conv weights reflect θ
end

# Flux.params(model) / gradient(θ) / Flux.Optimise.update!(opt, θ, ∇) (scripts/script.jl:84-86):
# the one trainable array is θ.  ADAM is elementwise, so training θ in the library layout is the
# same arithmetic as training the Flux layout; get_params / set_params! convert for checkpoints.
Flux.@functor HIPModel (θ,)
Flux.trainable(m::HIPModel) = (θ = m.θ,)

function param_count(cfg::ModelCfg)
    ne, nel = Ref{Clonglong}(), Ref{Clonglong}()
    check(ccall((:md2_arch_param_count, lib), Cint, (Ref{ModelCfg}, Ref{Clonglong}, Ref{Clonglong}),
                cfg, ne, nel))
    return Int(ne[]), Int(nel[])
end

# (name, shape, 0-based offset) of table entry i (0-based)
function param_info(cfg::ModelCfg, i)
    name = Vector{UInt8}(undef, 128); nd = Ref{Cint}(); shape = zeros(Cint, 4); off = Ref{Clonglong}()
    check(ccall((:md2_arch_param_info, lib), Cint,
                (Ref{ModelCfg}, Cint, Ptr{UInt8}, Cint, Ref{Cint}, Ptr{Cint}, Ref{Clonglong}),
                cfg, i, name, length(name), nd, shape, off))
    return unsafe_string(pointer(name)), Tuple(Int.(shape[1:nd[]])), Int(off[])
end

# Flux params -> the library's flat vector: conv weights (kw,kh,cin,cout) flipped in both spatial
# axes (true convolution -> cross-correlation); everything else copied as is.  `ps` iterates in
# Flux `params(model)` order, which is the table order.
function flat_params(cfg::ModelCfg, ps)
    ne, nel = param_count(cfg)
    flat = Vector{Float32}(undef, nel)
    for (i, p) in enumerate(ps)
        name, shape, off = param_info(cfg, i - 1)
        length(p) == prod(shape) || error("parameter $name: Flux size $(size(p)) vs table $shape")
        a = Array{Float32}(p)
        ndims(a) == 4 && (a = a[end:-1:1, end:-1:1, :, :])
        flat[off+1:off+length(a)] = vec(a)
    end
    ne == length(collect(ps)) || error("Flux model has a different parameter count than the table")
    return ROCVector{Float32}(flat)
end

function HIPModel(cfg::ModelCfg, θ::ROCVector{Float32})
    ∇θ = similar(θ); h = Ref{Ptr{Cvoid}}()
    check(ccall((:md2_model_create, lib), Cint,
                (Ref{ModelCfg}, Ptr{Float32}, Ptr{Float32}, Ref{Ptr{Cvoid}}), cfg, θ, ∇θ, h))
    m = HIPModel(h[], cfg, θ, ∇θ, fill!(similar(θ), 0), fill!(similar(θ), 0), 0, false)
    repack!(m)
    finalizer(x -> ccall((:md2_model_destroy, lib), Cint, (Ptr{Cvoid},), x.handle), m)
end

# after the caller changed m.θ in place (Flux.Optimise.update!, loading a checkpoint): re-pack the
# library's conv weights.  train_loss does it by itself after every pullback (see below).
function repack!(m::HIPModel)
    check(ccall((:md2_model_repack, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), m.handle, stream_ptr()))
    m.packed = true
    return m
end

# (m)(x, source_ids, target_id) -- disparities (Julia (w,h,1,n) views of library memory) and
# poses of the last forward (src/model.jl:24-55)
function outputs(m::HIPModel)
    d = Vector{Ptr{Float32}}(undef, 5); w = zeros(Cint, 5); h = zeros(Cint, 5); pose = Ref{Ptr{Float32}}()
    check(ccall((:md2_model_outputs, lib), Cint,
                (Ptr{Cvoid}, Ptr{Ptr{Float32}}, Ptr{Cint}, Ptr{Cint}, Ref{Ptr{Float32}}),
                m.handle, d, w, h, pose))
    n = m.cfg.batch
    np = m.cfg.embedding_levels > 0 ? Int(m.cfg.num_bins) : 1          # MPI: plane images
    disps = [unsafe_wrap(ROCArray, d[k], (Int(w[k]), Int(h[k]), 1, n * np)) for k in 1:m.cfg.n_levels]
    return disps, unsafe_wrap(ROCArray, pose[], (6, 2n))
end

"""
    HIPModel(model, cache, params; num_bins=32)

The HIP model of a reference `Model(encoder, depth_decoder, pose_decoder)` (src/model.jl:24-29,
built as in scripts/script.jl:77-81) for one `TrainCache` / `Params`: the architecture (ResNet
depth, input channels, `scale_levels`, `embedding_levels`) is read off the Flux model and its
parameters are copied (conv kernels flipped into the library layout) into the flat θ, and every
BatchNorm's running μ / σ² into the library's statistics (`set_bn_stats!`).
"""
function HIPModel(model, cache, params; num_bins=32)
    enc, dec = model.encoder, model.depth_decoder
    ch = collect(enc.stages)
    levels = cumsum([length(b) for b in dec.branches])
    emb = size(dec.branches[1][1].c1.d.weight, 3) - ch[end]
    ps = collect(Flux.params(model))
    in_ch = size(ps[1], 3)                         # the stem conv (kw,kh,cin,64)
    for arch in (ch[end] == 2048 ? (50,) : (18, 34))
        cfg = ModelCfg(arch, in_ch, levels, params, cache; embedding_levels=emb,
                       num_bins=emb > 0 ? num_bins : 1)
        param_count(cfg)[1] == length(ps) || continue
        m = HIPModel(cfg, flat_params(cfg, ps))
        # the BatchNorm running statistics (μ, σ²) are model state too: Flux.params holds γ and β only
        return set_bn_stats!(m, flat_bn_stats(cfg, model))
    end
    error("HIPModel: the Flux model matches no ResidualNetwork(18/34/50) + DepthDecoder + PoseDecoder table")
end

"""
    (m::HIPModel)(x, source_ids, target_id) -> (disparities, poses)

`(m::Model)(x, source_ids, target_id)` of src/model.jl:31-55 (called by train_loss at
src/training.jl:26 and bare at scripts/script.jl:93) on the HIP path, forward only: `disparities`
one (w,h,1,n) array per scale level ((w,h,1,n*num_bins) in MPI mode), `poses` one
`(rvec = (3,n), tvec = (3,1,n))` per source (the fields train_loss reads of `Pose`).  The rrule's
pullback runs the library's backward from the caller's cotangents (md2_model_backward_from), so
the reference's own train_loss can be differentiated through it by Zygote.  `source_ids` /
`target_id` must be the ones the model was built with.
"""
function (m::HIPModel)(x::ROCArray{Float32,5}, source_ids, target_id)
    (target_id - 1, source_ids[1] - 1, source_ids[2] - 1) == (m.cfg.target, m.cfg.src0, m.cfg.src1) ||
        error("HIPModel: target_id / source_ids differ from the config the model was built with")
    _forward(m, m.θ, x)
end

function _forward(m::HIPModel, θ::ROCVector{Float32}, x::ROCArray{Float32,5})
    θ === m.θ || error("HIPModel: θ must be the model's own parameter vector")
    m.packed || repack!(m)
    check(ccall((:md2_model_forward, lib), Cint,
                (Ptr{Cvoid}, Ptr{Float32}, Ptr{Ptr{Float32}}, Ptr{Ptr{Float32}}, Ptr{Cvoid}),
                m.handle, x, C_NULL, C_NULL, stream_ptr()))
    disps, pose = outputs(m)
    n = m.cfg.batch
    poses = [(rvec = pose[1:3, (s - 1) * n + 1:s * n], tvec = reshape(pose[4:6, (s - 1) * n + 1:s * n], 3, 1, n))
             for s in 1:2]
    return [copy(d) for d in disps], poses        # copies: the next forward reuses the buffers
end

function ChainRulesCore.rrule(::typeof(_forward), m::HIPModel, θ::ROCVector{Float32}, x)
    y = _forward(m, θ, x)
    function forward_pullback(Δ)
        Δd, Δp = unthunk(Δ[1]), unthunk(Δ[2])
        keep = Any[]
        dptrs = fill(Ptr{Float32}(C_NULL), 5)
        if !(Δd isa AbstractZero)
            for (k, d) in enumerate(Δd)
                d = unthunk(d)
                d isa AbstractZero && continue
                a = ROCArray{Float32}(d); push!(keep, a); dptrs[k] = pointer(a)
            end
        end
        dpose = Ptr{Float32}(C_NULL)
        if !(Δp isa AbstractZero)
            n = m.cfg.batch; P = fill!(ROCArray{Float32}(undef, 6, 2n), 0f0)
            for (s, p) in enumerate(Δp)
                p = unthunk(p)
                p isa AbstractZero && continue
                r, t = unthunk(p.rvec), unthunk(p.tvec)
                r isa AbstractZero || (P[1:3, (s - 1) * n + 1:s * n] .= reshape(r, 3, n))
                t isa AbstractZero || (P[4:6, (s - 1) * n + 1:s * n] .= reshape(t, 3, n))
            end
            push!(keep, P); dpose = pointer(P)
        end
        check(ccall((:md2_model_backward_from, lib), Cint,
                    (Ptr{Cvoid}, Ptr{Ptr{Float32}}, Ptr{Float32}, Ptr{Cvoid}),
                    m.handle, dptrs, dpose, stream_ptr()))
        AMDGPU.synchronize()                 # the cotangent copies in `keep` are read asynchronously
        m.packed = false
        return NoTangent(), NoTangent(), copy(m.∇θ), NoTangent()
    end
    return y, forward_pullback
end

# the loss-tail config of this model (for the visualisation pass)
function loss_cfg(m::HIPModel)
    c = m.cfg; disps, _ = outputs(m)
    LossCfg(c.batch, c.in_channels, c.width, c.height, c.n_levels,
            pad5([size(d, 1) for d in disps], Cint), pad5([size(d, 2) for d in disps], Cint),
            pad5([c.disparity_smoothness * s for s in c.scales[1:c.n_levels]], Cfloat),
            Float32(c.n_levels), 1, c.K, c.invK, c.min_depth, c.max_depth,
            3 * c.in_channels * c.height * c.width, c.in_channels * c.height * c.width,
            c.target, c.src0, c.src1, (c.src0 < c.target ? 1 : 0) | (c.src1 < c.target ? 2 : 0), 1)
end

"""
    train_loss(m, x, auto_loss, cache, params, do_visualization=false)

`train_loss` of src/training.jl:21-78 on the HIP path, with the reference's return convention:
`(loss, vis_disparity, vis_warped, vis_loss)` where `loss` is a host `Float32` scalar
(`loss / T(length(cache.scales))`, :77) and the visualisation outputs are host arrays
(`cpu(disparities[end])` (W,H,1,n), `cpu.(warped_images)` two (W,H,C,n), `cpu(warp_loss)`
(W,H,1,n); `nothing`s when `do_visualization` is false, :34-37,71-74).  The forward also runs the
fused loss-tail pullback; the rrule finishes the backward.  `cache` / `params` are the ones the
model was built with (md2_model_cfg): any field that differs raises (`check_config`).

Zygote: `gradient(() -> train_loss(m, x, ...)[1], Flux.params(m))` (the implicit-parameter loop
of scripts/script.jl:84-86, src/simple_depth.jl:25-42) returns the gradient under `m.θ`, in
m.θ's own layout, so `Flux.Optimise.update!(opt, Flux.params(m), ∇)` updates m.θ consistently.

`x_net` (like x, e.g. `color_jitter(x, params)`): the frames the networks see; the loss, SSIM and
the automask stay on x (md2_model_forward_loss_aug).  `nothing`: the plain call.
"""
function train_loss(m::HIPModel, x::ROCArray{Float32,5}, auto_loss, cache, params,
                    do_visualization::Bool=false; x_net=nothing)
    check_config(m, cache, params)
    x_net === nothing || size(x_net) == size(x) || error("x_net must have x's size")
    _train_loss(m, m.θ, x, auto_loss, do_visualization, x_net)     # m.θ read in traced code: accum_param
end

"""
    train_loss_stereo(m, x, x_stereo, stereo_Rt, auto_loss, cache, params; temporal=true, x_net=nothing)

`train_loss` with stereo supervision (md2_model_forward_loss_stereo): `x_stereo` (W,H,C,n) is the
other camera's frame at the target's time, `stereo_Rt` (12,n) its fixed transform
(`stereo_transforms`).  `temporal = true` is "MS", the loss over both temporal sources and the stereo
frame; `temporal = false` is "S", the stereo frame alone (the pose network's gradient is zero).
Returns `(loss, nothing, nothing, nothing)`; differentiable like `train_loss` (same rrule).
"""
function train_loss_stereo(m::HIPModel, x::ROCArray{Float32,5}, x_stereo::ROCArray{Float32,4},
                           stereo_Rt::ROCArray{Float32,2}, auto_loss, cache, params; temporal::Bool=true,
                           x_net=nothing)
    check_config(m, cache, params)
    x_net === nothing || size(x_net) == size(x) || error("x_net must have x's size")
    W, H, C, _, n = size(x)
    size(x_stereo) == (W, H, C, n) || error("x_stereo must be (W,H,C,n) = ", (W, H, C, n))
    size(stereo_Rt) == (12, n) || error("stereo_Rt must be (12,n) = ", (12, n))
    _train_loss(m, m.θ, x, auto_loss, false, x_net, (x = x_stereo, Rt = stereo_Rt, temporal = temporal))
end

# The executor's kernels, buffers and loss-tail weights are built for ONE (Params, TrainCache)
# (md2_model_cfg).  The reference reads them per call (src/training.jl:40-67), so a caller passing
# a different cache / params must get an error, not the build-time config's loss.
function check_config(m::HIPModel, cache, params)
    c = m.cfg
    bad = String[]
    (params.batch_size, params.target_size...) == (c.batch, c.width, c.height) ||
        push!(bad, "batch_size / target_size")
    Float32(params.min_depth) == c.min_depth && Float32(params.max_depth) == c.max_depth ||
        push!(bad, "min_depth / max_depth")
    Float32(params.disparity_smoothness) == c.disparity_smoothness || push!(bad, "disparity_smoothness")
    Cint(params.automasking) == c.automasking || push!(bad, "automasking")
    (cache.target_id - 1, cache.source_ids[1] - 1, cache.source_ids[2] - 1) == (c.target, c.src0, c.src1) ||
        push!(bad, "target_id / source_ids")
    Float32.(cache.scales) == collect(c.scales[1:c.n_levels]) || push!(bad, "scales")
    rowmajor(cache.K) == c.K && rowmajor(cache.invK) == c.invK || push!(bad, "K / invK")
    isempty(bad) || error("train_loss: ", join(bad, ", "), " differ from the config the HIPModel was ",
                          "built with (md2_model_cfg); build a HIPModel for this cache / params")
    return nothing
end

function _train_loss(m::HIPModel, θ::ROCVector{Float32}, x::ROCArray{Float32,5}, auto_loss,
                     do_visualization::Bool, x_net=nothing, stereo=nothing)
    θ === m.θ || error("train_loss: θ must be the model's own parameter vector")
    m.packed || repack!(m)               # θ may have been updated in place since the last step
    loss = ROCVector{Float32}(undef, 1)
    if stereo !== nothing                # MS (temporal) or S: the loss and the automask read stereo.x
        check(ccall((:md2_model_forward_loss_stereo, lib), Cint,
                    (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cint, Ptr{Float32},
                     Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
                    m.handle, x, ptr(x_net), stereo.x, stereo.Rt, stereo.temporal ? 1 : 0, ptr(auto_loss), loss,
                    C_NULL, stream_ptr()))
    elseif x_net === nothing
        check(ccall((:md2_model_forward_loss, lib), Cint,
                    (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
                    m.handle, x, ptr(auto_loss), loss, C_NULL, stream_ptr()))
    else
        check(ccall((:md2_model_forward_loss_aug, lib), Cint,
                    (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
                    m.handle, x, x_net, ptr(auto_loss), loss, C_NULL, stream_ptr()))
    end
    l = Array(loss)[1]                   # host scalar, as the reference's mean(...) / T(...)
    do_visualization || return (l, nothing, nothing, nothing)
    disps, pose = outputs(m)
    cfg = loss_cfg(m); n = m.cfg.batch; c = m.cfg.in_channels; W = m.cfg.width; H = m.cfg.height
    vis_loss = ROCArray{Float32}(undef, W, H, n, cfg.nscales)
    vis_sel = ROCArray{Int8}(undef, W, H, n, cfg.nscales)
    vis_warped = ROCArray{Float32}(undef, W, H, c, n, 2)
    tmp = ROCVector{Float32}(undef, 1)
    ws = ROCVector{UInt8}(undef, ccall((:md2_loss_workspace_size, lib), Csize_t, (Ref{LossCfg},), cfg))
    out = LossOut(pointer(tmp), C_NULL, ntuple(_ -> Ptr{Float32}(C_NULL), 5), C_NULL,
                  pointer(vis_loss), pointer(vis_sel), pointer(vis_warped), C_NULL)
    dptrs = [pointer(d) for d in disps]
    check(ccall((:md2_loss_fwd_bwd, lib), Cint,
                (Ref{LossCfg}, Ptr{Ptr{Float32}}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat,
                 Ref{LossOut}, Ptr{UInt8}, Ptr{Cvoid}),
                cfg, dptrs, pose, x, ptr(auto_loss), 1f0, out, ws, stream_ptr()))
    # training.jl:34-37,71-74: last disparity, both warped sources and the last scale's loss map
    return (l, Array(disps[end]), (Array(vis_warped[:, :, :, :, 1]), Array(vis_warped[:, :, :, :, 2])),
            Array(reshape(vis_loss[:, :, :, end], W, H, 1, n)))
end

# gradient(θ) do train_loss(...)[1] end: the remaining backward segments -> m.∇θ.  `bucket(off,
# len)` runs after each segment (that flat range is final) so a DP caller can all-reduce it.
function gradient!(m::HIPModel; bucket=(off, len) -> nothing)
    nseg = ccall((:md2_model_num_segments, lib), Cint, (Ptr{Cvoid},), m.handle)
    off, len = Ref{Clonglong}(), Ref{Clonglong}()
    for k in 0:nseg-1
        check(ccall((:md2_model_backward_segment, lib), Cint,
                    (Ptr{Cvoid}, Cint, Ref{Clonglong}, Ref{Clonglong}, Ptr{Cvoid}),
                    m.handle, k, off, len, stream_ptr()))
        bucket(off[], len[])
    end
    return m.∇θ
end

# Zygote: d(train_loss(...)[1])/dθ.  The loss cotangent enters the library's backward itself
# (md2_model_loss_cotangent scales the fused loss tail's d disp / d pose before segment 0).  The
# θ tangent is a fresh array in θ's own (library) layout -- what Flux.Optimise.update! adds to
# θ; the Flux-layout gradient (true-convolution kernels) is flux_gradient(m).  The caller is
# expected to update θ next, so the packed weights are marked stale (re-packed by the next
# train_loss, or already by the library's own update!).
function ChainRulesCore.rrule(::typeof(_train_loss), m::HIPModel, θ::ROCVector{Float32}, x, auto_loss,
                              do_visualization::Bool, x_net=nothing, stereo=nothing)
    y = _train_loss(m, θ, x, auto_loss, do_visualization, x_net, stereo)
    function train_loss_pullback(Δ)
        Δl = unthunk(Δ[1])
        Δl = Δl isa AbstractZero ? 0f0 : Float32(Δl)
        check(ccall((:md2_model_loss_cotangent, lib), Cint, (Ptr{Cvoid}, Cfloat, Ptr{Cvoid}),
                    m.handle, Δl, stream_ptr()))
        gradient!(m)
        m.packed = false
        return (NoTangent(), NoTangent(), copy(m.∇θ), NoTangent(), NoTangent(), NoTangent(), NoTangent(), NoTangent())
    end
    return y, train_loss_pullback
end

# the last gradient in Flux layout (Flux.params order, conv kernels as true convolutions): what
# Zygote returns for a Flux Model's params -- for comparing against / exporting to the reference
function flux_gradient(m::HIPModel)
    ∇flux = similar(m.∇θ)
    check(ccall((:md2_model_get_grads, lib), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Cvoid}),
                m.handle, ∇flux, stream_ptr()))
    return ∇flux
end

# Flux-layout parameters in / out of the model (device copies with the conv taps flipped)
function set_params!(m::HIPModel, flux::ROCVector{Float32})
    check(ccall((:md2_model_set_params, lib), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Cvoid}),
                m.handle, flux, stream_ptr()))
    m.packed = true                      # md2_model_set_params re-packs
    return m
end
function get_params(m::HIPModel)
    flux = similar(m.θ)
    check(ccall((:md2_model_get_params, lib), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Cvoid}),
                m.handle, flux, stream_ptr()))
    return flux
end

# ------------------------------------------------------------------------------------------------
# BatchNorm running statistics and test mode.  Flux keeps μ / σ² in the BatchNorm layers (not in
# Flux.params); the library keeps them as one flat vector: per BatchNorm, in the order of its
# gamma entry in the parameter table, C means then C variances (md2_model_get_bn_stats).
# ------------------------------------------------------------------------------------------------
function bn_stat_count(cfg::ModelCfg)
    nb, nel = Ref{Clonglong}(), Ref{Clonglong}()
    check(ccall((:md2_arch_bn_stat_count, lib), Cint, (Ref{ModelCfg}, Ref{Clonglong}, Ref{Clonglong}),
                cfg, nb, nel))
    return Int(nb[]), Int(nel[])
end

function bn_stats(m::HIPModel)
    v = ROCVector{Float32}(undef, bn_stat_count(m.cfg)[2])
    check(ccall((:md2_model_get_bn_stats, lib), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Cvoid}),
                m.handle, v, stream_ptr()))
    return v
end

# a negative variance or a non-finite entry is refused (MD2_EINVAL; the model's state is unchanged)
function set_bn_stats!(m::HIPModel, v::ROCVector{Float32})
    length(v) == bn_stat_count(m.cfg)[2] || error("set_bn_stats!: $(length(v)) elements, the model needs ",
                                                   bn_stat_count(m.cfg)[2])
    check(ccall((:md2_model_set_bn_stats, lib), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Cvoid}),
                m.handle, v, stream_ptr()))
    return m
end

# the BatchNorm layers of a Flux model in Flux.params order (the same depth-first walk over
# Flux.trainable that params! does), i.e. the order of the table's gamma entries
function batchnorms!(out, x)
    x isa Flux.BatchNorm && return push!(out, x)
    x isa AbstractArray{<:Number} && return out
    for c in Flux.trainable(x)
        batchnorms!(out, c)
    end
    return out
end

# μ / σ² of every Flux BatchNorm of `model` as the library's flat vector
function flat_bn_stats(cfg::ModelCfg, model)
    bns = batchnorms!(Any[], model)
    nb, nel = bn_stat_count(cfg)
    length(bns) == nb || error("Flux model has $(length(bns)) BatchNorm layers, the table has $nb")
    flat = Float32[]
    for b in bns
        append!(flat, Array{Float32}(b.μ)); append!(flat, Array{Float32}(b.σ²))
    end
    length(flat) == nel || error("BatchNorm statistics: $(length(flat)) elements, the table has $nel")
    return ROCVector{Float32}(flat)
end

"""
    testmode!(m::HIPModel, on=true); trainmode!(m)

Flux `testmode!` / `trainmode!` on the HIP path.  While on, `eval_disparity(m, x)` and
`m(x, source_ids, target_id)` normalise with the running statistics (each BatchNorm folded into the
conv before it; the statistics are not modified) and every training call fails with MD2_ESTATE.
If m.θ was changed in place since the last pack, the switch re-packs (and so folds the new weights).
"""
function testmode!(m::HIPModel, on=true)
    on && !m.packed && repack!(m)
    check(ccall((:md2_model_set_testmode, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}),
                m.handle, on ? 1 : 0, stream_ptr()))
    return m
end
trainmode!(m::HIPModel) = testmode!(m, false)
istestmode(m::HIPModel) = ccall((:md2_model_testmode, lib), Cint, (Ptr{Cvoid},), m.handle) != 0

# update!(ADAM(η), θ, ∇θ) -- Flux ADAM, β = (0.9, 0.999), ε = 1e-8 (scripts/script.jl:85)
function update!(m::HIPModel, η; β=(0.9f0, 0.999f0), ϵ=1f-8, grad_scale=1f0)
    m.step += 1
    check(ccall((:md2_model_adam, lib), Cint,
                (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Cfloat, Cfloat, Cfloat, Cfloat, Cint, Cfloat, Ptr{Cvoid}),
                m.handle, m.m, m.v, η, β[1], β[2], ϵ, m.step, grad_scale, stream_ptr()))
    m.packed = true                      # md2_model_adam re-packs
    return m
end

"""
    set_grad_guard(m::HIPModel, on::Bool; max_norm=Inf32)
    grad_guard_state(m::HIPModel)

The guarded optimiser step (md2_model_set_grad_guard).  While on, `update!`, `train_step!` and the
captured and data-parallel steps measure the global L2 norm of ∇θ on the device, clip it to
`max_norm` (`Inf32`: no clipping) and leave θ and the ADAM moments untouched when a gradient entry is
NaN or Inf.  A skipped step still counts in `m.step`; BatchNorm running statistics moved in the
forward stay moved.  Switching clears `skipped` and synchronises the device.

`grad_guard_state` copies the 40-byte device state to the host (this synchronises) and returns
`(norm, coef, ok, skipped, nonfinite)` of the last guarded step.
"""
function set_grad_guard(m::HIPModel, on::Bool; max_norm=Inf32)
    check(ccall((:md2_model_set_grad_guard, lib), Cint, (Ptr{Cvoid}, Cint, Cfloat),
                m.handle, on ? 1 : 0, Float32(max_norm)))
    return m
end

function grad_guard_state(m::HIPModel)
    p = Ref{Ptr{UInt8}}(C_NULL)
    check(ccall((:md2_model_grad_guard_state, lib), Cint, (Ptr{Cvoid}, Ptr{Ptr{UInt8}}), m.handle, p))
    raw = Array(unsafe_wrap(ROCArray, p[], (40,)))         # md2_guard_state: f64, i64, i64, 3 x f32, i32
    f(T, off) = reinterpret(T, raw[off + 1:off + sizeof(T)])[1]
    return (norm=f(Float32, 24), coef=f(Float32, 28), ok=f(Int32, 36) != 0, skipped=f(Int64, 16),
            nonfinite=f(Int64, 8))
end

# eval_disparity(m, x) -- src/model.jl:63; x::(W,H,C,n), n <= batch
function eval_disparity(m::HIPModel, x::ROCArray{Float32,4})
    d = Vector{Ptr{Float32}}(undef, 5)
    check(ccall((:md2_model_eval_disparity, lib), Cint,
                (Ptr{Cvoid}, Ptr{Float32}, Cint, Ptr{Ptr{Float32}}, Ptr{Cvoid}),
                m.handle, x, size(x, 4), d, stream_ptr()))
    W, H = m.cfg.width, m.cfg.height; lv = m.cfg.scale_levels
    return [unsafe_wrap(ROCArray, d[k], (W >> (5 - lv[k]), H >> (5 - lv[k]), 1, size(x, 4)))
            for k in 1:m.cfg.n_levels]
end

# eval_pose(m, x) -- the PoseDecoder on the consecutive frames of x::(W,H,C,n), 2 <= n <= 2*batch+1,
# without the DepthDecoder: (6, n-1), column i = the raw (rvec, tvec) of the pair (frame i, frame i+1).
# Wraps an executor-owned buffer that the model's next forward overwrites: copy to keep.
function eval_pose(m::HIPModel, x::ROCArray{Float32,4})
    p = Ref{Ptr{Float32}}(C_NULL)
    check(ccall((:md2_model_eval_pose, lib), Cint,
                (Ptr{Cvoid}, Ptr{Float32}, Cint, Ptr{Ptr{Float32}}, Ptr{Cvoid}),
                m.handle, x, size(x, 4), p, stream_ptr()))
    return unsafe_wrap(ROCArray, p[], (6, size(x, 4) - 1))
end

# ------------------------------------------------------------------------------------------------
# Op-level forward + rrule pairs (src/utils.jl, src/training.jl): for callers that keep Flux for
# the networks and differentiate the loss ops one at a time.
# ------------------------------------------------------------------------------------------------
struct SSIM end                                        # src/utils.jl:17-43 (constants built in)

function (s::SSIM)(x::ROCArray{Float32,4}, y::ROCArray{Float32,4})
    W, H, C, N = size(x); out = similar(x)
    check(ccall((:md2_ssim_fwd, lib), Cint,
                (Ptr{Float32}, Ptr{Float32}, Cint, Cint, Cint, Cint, Ptr{Float32}, Ptr{Cvoid}),
                x, y, N, C, H, W, out, stream_ptr()))
    return out
end

function ChainRulesCore.rrule(s::SSIM, x::ROCArray{Float32,4}, y::ROCArray{Float32,4})
    out = s(x, y)
    function ssim_pullback(Δ)
        W, H, C, N = size(x); dx = similar(x); dy = similar(y)
        dout = ROCArray{Float32}(unthunk(Δ))
        check(ccall((:md2_ssim_bwd, lib), Cint,
                    (Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cint, Cint, Cint, Cint, Ptr{Float32},
                     Ptr{Float32}, Ptr{Cvoid}), x, y, dout, N, C, H, W, dx, dy, stream_ptr()))
        return NoTangent(), dx, dy
    end
    return out, ssim_pullback
end

# Backproject: (b)(depth (1, W*H, N), invK) -> (3, W*H, N)   src/utils.jl:45-69
struct Backproject; width::Int; height::Int; end
function (b::Backproject)(depth::ROCArray{Float32,3}, invK)
    N = size(depth, 3); out = ROCArray{Float32}(undef, 3, b.width * b.height, N)
    iK = collect(rowmajor(invK))
    check(ccall((:md2_backproject_fwd, lib), Cint,
                (Ptr{Float32}, Cint, Cint, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
                depth, N, b.width, b.height, iK, out, stream_ptr()))
    return out
end
function ChainRulesCore.rrule(b::Backproject, depth::ROCArray{Float32,3}, invK)
    out = b(depth, invK)
    function backproject_pullback(Δ)
        dd = similar(depth); dout = ROCArray{Float32}(unthunk(Δ)); iK = collect(rowmajor(invK))
        check(ccall((:md2_backproject_bwd, lib), Cint,
                    (Ptr{Float32}, Cint, Cint, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
                    dout, size(depth, 3), b.width, b.height, iK, dd, stream_ptr()))
        return NoTangent(), dd, NoTangent()            # invK: TrainCache constant
    end
    return out, backproject_pullback
end

# Project: (p)(points (3, W*H, N), K, R (3,3,N), t (3,1,N)) -> (2, W, H, N)   src/utils.jl:71-103
struct Project; width::Int; height::Int; end
rowmajor_batch(R) = ROCArray{Float32}(permutedims(Array(R), (2, 1, 3)))   # [n][3][3] row-major
function (p::Project)(points::ROCArray{Float32,3}, K, R, t)
    N = size(points, 3); out = ROCArray{Float32}(undef, 2, p.width, p.height, N)
    check(ccall((:md2_project_fwd, lib), Cint,
                (Ptr{Float32}, Cint, Cint, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
                points, N, p.width, p.height, collect(rowmajor(K)), rowmajor_batch(R),
                ROCArray{Float32}(t), out, stream_ptr()))
    return out
end
function ChainRulesCore.rrule(p::Project, points::ROCArray{Float32,3}, K, R, t)
    out = p(points, K, R, t)
    function project_pullback(Δ)
        N = size(points, 3); dpts = similar(points)
        dRr = ROCArray{Float32}(undef, 9, N); dt = ROCArray{Float32}(undef, 3, 1, N)
        ws = ROCVector{UInt8}(undef, ccall((:md2_project_workspace_size, lib), Csize_t,
                                           (Cint, Cint, Cint), N, p.width, p.height))
        check(ccall((:md2_project_bwd, lib), Cint,
                    (Ptr{Float32}, Cint, Cint, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Float32},
                     Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{UInt8}, Ptr{Cvoid}),
                    points, N, p.width, p.height, collect(rowmajor(K)), rowmajor_batch(R),
                    ROCArray{Float32}(t), ROCArray{Float32}(unthunk(Δ)), dpts, dRr, dt, ws, stream_ptr()))
        dR = permutedims(reshape(dRr, 3, 3, N), (2, 1, 3))   # back to column-major (3,3,N)
        return NoTangent(), dpts, NoTangent(), dR, dt
    end
    return out, project_pullback
end

# grid_sample(x, grid; padding_mode=:border), align_corners=true -- src/training.jl:56
function grid_sample_border(x::ROCArray{Float32,4}, grid::ROCArray{Float32,4})
    Wi, Hi, C, N = size(x); Wo, Ho = size(grid, 2), size(grid, 3)
    out = ROCArray{Float32}(undef, Wo, Ho, C, N)
    check(ccall((:md2_grid_sample_border_fwd, lib), Cint,
                (Ptr{Float32}, Ptr{Float32}, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float32}, Ptr{Cvoid}),
                x, grid, N, C, Hi, Wi, Ho, Wo, out, stream_ptr()))
    return out
end
function ChainRulesCore.rrule(::typeof(grid_sample_border), x::ROCArray{Float32,4}, grid::ROCArray{Float32,4})
    out = grid_sample_border(x, grid)
    function grid_sample_pullback(Δ)
        Wi, Hi, C, N = size(x); Wo, Ho = size(grid, 2), size(grid, 3)
        dgrid = similar(grid); dx = fill!(similar(x), 0)
        check(ccall((:md2_grid_sample_border_bwd, lib), Cint,
                    (Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cint, Cint, Cint, Cint, Cint, Cint,
                     Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
                    x, grid, ROCArray{Float32}(unthunk(Δ)), N, C, Hi, Wi, Ho, Wo, dgrid, dx, stream_ptr()))
        return NoTangent(), dx, dgrid
    end
    return out, grid_sample_pullback
end

# smooth_loss(disparity (W,H,N), image (W,H,C,N)) -> scalar   src/utils.jl:163-177
function smooth_loss(disp::ROCArray{Float32}, img::ROCArray{Float32,4})
    W, H, C, N = size(img); loss = ROCVector{Float32}(undef, 1)
    ws = ROCVector{UInt8}(undef, ccall((:md2_smooth_loss_workspace_size, lib), Csize_t, (Cint, Cint, Cint), N, W, H))
    check(ccall((:md2_smooth_loss_fwd, lib), Cint,
                (Ptr{Float32}, Ptr{Float32}, Cint, Cint, Cint, Cint, Ptr{Float32}, Ptr{UInt8}, Ptr{Cvoid}),
                disp, img, N, C, H, W, loss, ws, stream_ptr()))
    return Array(loss)[1]
end
function ChainRulesCore.rrule(::typeof(smooth_loss), disp::ROCArray{Float32}, img::ROCArray{Float32,4})
    l = smooth_loss(disp, img)
    function smooth_loss_pullback(Δ)
        W, H, C, N = size(img); dd = similar(disp)
        ws = ROCVector{UInt8}(undef, ccall((:md2_smooth_loss_workspace_size, lib), Csize_t, (Cint, Cint, Cint), N, W, H))
        check(ccall((:md2_smooth_loss_bwd, lib), Cint,
                    (Ptr{Float32}, Ptr{Float32}, Cint, Cint, Cint, Cint, Cfloat, Ptr{Float32}, Ptr{UInt8}, Ptr{Cvoid}),
                    disp, img, N, C, H, W, Float32(unthunk(Δ)), dd, ws, stream_ptr()))
        return NoTangent(), dd, NoTangent()
    end
    return l, smooth_loss_pullback
end

# One scale of train_loss's loop body (src/training.jl:43-62): upsample -> depth -> Backproject ->
# Project -> grid_sample -> photometric_loss -> min over sources [-> _apply_mask].
# disp (dw,dh,1,N); Rt (12, N, 2) = composeT outputs (R row-major, t); x (W,H,C,3,N).
function warp_photometric(cfg::WarpCfg, disp, Rt, x, automask=nothing)
    loss = ROCArray{Float32}(undef, cfg.width, cfg.height, 1, cfg.n)
    ws = ROCVector{UInt8}(undef, ccall((:md2_warp_photometric_workspace_size, lib), Csize_t, (Ref{WarpCfg},), cfg))
    check(ccall((:md2_warp_photometric_fwd, lib), Cint,
                (Ref{WarpCfg}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32},
                 Ptr{Int8}, Ptr{UInt8}, Ptr{Cvoid}),
                cfg, disp, Rt, x, ptr(automask), loss, C_NULL, ws, stream_ptr()))
    return loss
end
function ChainRulesCore.rrule(::typeof(warp_photometric), cfg::WarpCfg, disp, Rt, x, automask=nothing)
    loss = warp_photometric(cfg, disp, Rt, x, automask)
    function warp_photometric_pullback(Δ)
        dd = similar(disp); dRt = similar(Rt)
        ws = ROCVector{UInt8}(undef, ccall((:md2_warp_photometric_workspace_size, lib), Csize_t, (Ref{WarpCfg},), cfg))
        check(ccall((:md2_warp_photometric_bwd, lib), Cint,
                    (Ref{WarpCfg}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32},
                     Ptr{Float32}, Ptr{Float32}, Ptr{UInt8}, Ptr{Cvoid}),
                    cfg, disp, Rt, x, ptr(automask), ROCArray{Float32}(unthunk(Δ)), dd, dRt, ws, stream_ptr()))
        return NoTangent(), NoTangent(), dd, dRt, NoTangent(), NoTangent()
    end
    return loss, warp_photometric_pullback
end

# composeT(so3_exp_map(rvec), tvec, invert) for the 2n poses (src/utils.jl:106-145,185-192);
# pose (6, 2n) = (rvec, tvec) per (source, sample); bit s of invert_mask: source s < target.
function so3_compose(pose::ROCArray{Float32,2}, invert_mask::Integer)
    n = size(pose, 2) ÷ 2; Rt = ROCArray{Float32}(undef, 12, 2n)
    check(ccall((:md2_so3_compose_fwd, lib), Cint, (Ptr{Float32}, Cint, Cint, Ptr{Float32}, Ptr{Cvoid}),
                pose, n, invert_mask, Rt, stream_ptr()))
    return Rt
end
function ChainRulesCore.rrule(::typeof(so3_compose), pose::ROCArray{Float32,2}, invert_mask::Integer)
    Rt = so3_compose(pose, invert_mask)
    function so3_compose_pullback(Δ)
        dpose = similar(pose)
        check(ccall((:md2_so3_compose_bwd, lib), Cint,
                    (Ptr{Float32}, Cint, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
                    pose, size(pose, 2) ÷ 2, invert_mask, ROCArray{Float32}(unthunk(Δ)), dpose, stream_ptr()))
        return NoTangent(), dpose, NoTangent()
    end
    return Rt, so3_compose_pullback
end

# find_static(dataset, α) -- src/dtk.jl:51-69: per-triplet mean identity-reprojection loss of a
# batch x (W,H,C,3,n) on the GPU; the dataset keeps the files whose score exceeds α
function static_scores(x::ROCArray{Float32,5}; target_id=2, source_ids=(1, 3))
    W, H, C, L, n = size(x); scores = ROCVector{Float32}(undef, n)
    ws = ROCVector{UInt8}(undef, ccall((:md2_static_scores_workspace_size, lib), Csize_t, (Cint, Cint, Cint), n, H, W))
    check(ccall((:md2_static_scores, lib), Cint,
                (Ptr{Float32}, Cint, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Float32}, Ptr{UInt8}, Ptr{Cvoid}),
                x, n, C, H, W, target_id - 1, source_ids[1] - 1, source_ids[2] - 1, scores, ws, stream_ptr()))
    return Array(scores)
end

# Stereo supervision (include/md2.h, "Loss tail over S sources"): the loss tail over the two temporal
# sources of x (learned poses) and a stereo frame with a fixed transform ("MS", temporal = true), or
# over the stereo frame alone ("S").  x (W,H,C,3,n); x_stereo (W,H,C,n); stereo_Rt (12,n) from
# stereo_transforms; disps as the model emits them; pose (6,2n) (not read in S mode).
# Returns (loss, d_disp, d_pose) on the device, d_pose (6,2n) or nothing in S mode.  Data-only
# arguments; the caller chains d_disp / d_pose into the model's pullback.
"""
    stereo_transforms(sides, flips; baseline = 0.1f0)

(12, n) Float32: R = I (row-major) and t = (side_sign * flip_sign * baseline, 0, 0) per sample;
side_sign is -1 for a left-camera target (`:l`) and +1 for a right one, flip_sign -1 for a mirrored
sample -- Monodepth2's `stereo_T[0, 3] = side_sign * baseline_sign * 0.1`.  0.1 against KITTI's
0.54 m baseline is the `scale = 5.4` of `depth_errors(...; median_scaling=false)`.
"""
function stereo_transforms(sides, flips; baseline = 0.1f0)
    length(sides) == length(flips) || error("sides and flips differ in length")
    Rt = zeros(Float32, 12, length(sides))
    for (i, (s, f)) in enumerate(zip(sides, flips))
        s in (:l, :r) || error("side must be :l or :r")
        Rt[1, i] = Rt[5, i] = Rt[9, i] = 1f0
        Rt[10, i] = (s == :l ? -1f0 : 1f0) * (f ? -1f0 : 1f0) * Float32(baseline)
    end
    return Rt
end

function stereo_sources(x::ROCArray{Float32,5}, x_stereo::ROCArray{Float32,4}, stereo_Rt::ROCArray{Float32,2},
                        target_id, source_ids, temporal::Bool)
    W, H, C, L, n = size(x)
    size(x_stereo) == (W, H, C, n) || error("x_stereo must be (W,H,C,n) = ", (W, H, C, n))
    size(stereo_Rt) == (12, n) || error("stereo_Rt must be (12,n) = ", (12, n))
    fs = W * H * C
    src = LossSource[]
    if temporal
        length(source_ids) == 2 || error("two temporal sources")
        for (k, sid) in enumerate(source_ids)
            push!(src, LossSource(pointer(x) + 4 * (sid - 1) * fs, L * fs, k - 1, sid < target_id ? 1 : 0, C_NULL))
        end
    end
    push!(src, LossSource(pointer(x_stereo), fs, -1, 0, pointer(stereo_Rt)))
    return src
end

function automasking_loss_sources(x::ROCArray{Float32,5}, x_stereo::ROCArray{Float32,4}; target_id=2,
                                  source_ids=(1, 3), temporal::Bool=true)
    W, H, C, L, n = size(x); fs = W * H * C
    src = stereo_sources(x, x_stereo, ROCArray(zeros(Float32, 12, n)), target_id, source_ids, temporal)
    out = ROCArray{Float32}(undef, W, H, 1, n)
    check(ccall((:md2_automasking_loss_sources, lib), Cint,
                (Cint, Ptr{LossSource}, Ptr{Float32}, Clonglong, Cint, Cint, Cint, Cint, Ptr{Float32}, Ptr{Cvoid}),
                length(src), src, pointer(x) + 4 * (target_id - 1) * fs, L * fs, n, C, H, W, out, stream_ptr()))
    return out
end

# K / invK (both or neither): per-sample intrinsics, (9, n) each -- column i is sample i's 3x3 in
# row-major order, vec(K_i') -- md2_loss_fwd_bwd_sources_k; cfg.K / cfg.invK are then not read
function loss_tail_sources(cfg::LossCfg, disps, pose, x::ROCArray{Float32,5}, x_stereo::ROCArray{Float32,4},
                           stereo_Rt::ROCArray{Float32,2}, auto_loss; target_id=2, source_ids=(1, 3),
                           temporal::Bool=true, dloss=1f0,
                           K::Union{Nothing,ROCArray{Float32,2}}=nothing,
                           invK::Union{Nothing,ROCArray{Float32,2}}=nothing)
    W, H, C, L, n = size(x); fs = W * H * C
    (K === nothing) == (invK === nothing) || error("K and invK come together")
    K === nothing || (size(K) == (9, n) && size(invK) == (9, n)) || error("K and invK must be (9,n) = ", (9, n))
    src = stereo_sources(x, x_stereo, stereo_Rt, target_id, source_ids, temporal)
    nsrc = length(src)
    loss = ROCVector{Float32}(undef, 1)
    d_disp = [similar(d) for d in disps]
    d_pose = temporal ? ROCArray{Float32}(undef, 6, 2n) : nothing
    ws = ROCVector{UInt8}(undef, ccall((:md2_loss_sources_workspace_size, lib), Csize_t, (Ref{LossCfg}, Cint), cfg, nsrc))
    out = LossOut(pointer(loss), C_NULL, ntuple(i -> i <= length(d_disp) ? pointer(d_disp[i]) : Ptr{Float32}(C_NULL), 5),
                  temporal ? pointer(d_pose) : C_NULL, C_NULL, C_NULL, C_NULL, C_NULL)
    dptrs = [pointer(d) for d in disps]
    if K !== nothing
        check(ccall((:md2_loss_fwd_bwd_sources_k, lib), Cint,
                    (Ref{LossCfg}, Cint, Ptr{LossSource}, Ptr{Float32}, Clonglong, Ptr{Float32}, Ptr{Float32},
                     Ptr{Ptr{Float32}}, Ptr{Float32}, Ptr{Float32}, Cfloat, Ref{LossOut}, Ptr{UInt8}, Ptr{Cvoid}),
                    cfg, nsrc, src, pointer(x) + 4 * (target_id - 1) * fs, L * fs, K, invK, dptrs,
                    temporal ? pointer(pose) : C_NULL, ptr(auto_loss), Float32(dloss), out, ws, stream_ptr()))
        return loss, d_disp, d_pose
    end
    check(ccall((:md2_loss_fwd_bwd_sources, lib), Cint,
                (Ref{LossCfg}, Cint, Ptr{LossSource}, Ptr{Float32}, Clonglong, Ptr{Ptr{Float32}}, Ptr{Float32},
                 Ptr{Float32}, Cfloat, Ref{LossOut}, Ptr{UInt8}, Ptr{Cvoid}),
                cfg, nsrc, src, pointer(x) + 4 * (target_id - 1) * fs, L * fs, dptrs, temporal ? pointer(pose) : C_NULL,
                ptr(auto_loss), Float32(dloss), out, ws, stream_ptr()))
    return loss, d_disp, d_pose
end

# Depth evaluation (Monodepth2 / Eigen protocol; include/md2.h states every step): disparities
# disp (w,h,n) or (w,h,1,n) against ground-truth depth gt (Wg,Hg,n), one batched call, no host
# sync.  crop: :garg, nothing (whole image) or 0-based half-open (y0, y1, x0, x1) in gt pixels.
# Returns device arrays metrics (10, n) = abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, ratio,
# med_gt, med_pred per image, and counts (2, n) = count, n_bad.  Data only: no rrule.
garg_crop(gt_h, gt_w) = (floor(Int, 0.40810811 * gt_h), floor(Int, 0.99189189 * gt_h),
                         floor(Int, 0.03594771 * gt_w), floor(Int, 0.96405229 * gt_w))
function depth_errors(disp::ROCArray{Float32}, gt::ROCArray{Float32,3}; crop=:garg, min_depth=0.1f0,
                      max_depth=100f0, eval_min=1f-3, eval_max=80f0, median_scaling=true, scale=1f0)
    (ndims(disp) == 3 || (ndims(disp) == 4 && size(disp, 3) == 1)) || error("disp must be (w,h,n) or (w,h,1,n)")
    w, h = size(disp, 1), size(disp, 2); n = size(disp, ndims(disp))
    Wg, Hg = size(gt, 1), size(gt, 2)
    n == size(gt, 3) || error("batch mismatch: disp has ", n, " images, gt ", size(gt, 3))
    y0, y1, x0, x1 = crop === :garg ? garg_crop(Hg, Wg) : crop === nothing ? (0, Hg, 0, Wg) : crop
    cfg = DepthEvalCfg(n, h, w, Hg, Wg, y0, y1, x0, x1, min_depth, max_depth, eval_min, eval_max,
                       median_scaling ? 1 : 0, scale)
    nbytes = ccall((:md2_depth_eval_workspace_size, lib), Csize_t, (Ref{DepthEvalCfg},), cfg)
    ws = ROCVector{UInt8}(undef, max(nbytes, 256))      # an invalid cfg has size 0: the call says why
    metrics = ROCArray{Float32}(undef, 10, n); counts = ROCArray{Int32}(undef, 2, n)
    check(ccall((:md2_depth_eval, lib), Cint,
                (Ref{DepthEvalCfg}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Int32}, Ptr{UInt8}, Ptr{Cvoid}),
                cfg, disp, gt, metrics, counts, ws, stream_ptr()))
    return metrics, counts
end

# Ground-truth depth maps from LiDAR scans (include/md2.h states every operation): points (4, M)
# = x, y, z, reflectance per column; offsets: n+1 0-based host offsets, scan i = columns
# offsets[i]+1 .. offsets[i+1]; P: the row-major 3x4 velodyne -> image matrices as the C side reads
# them, i.e. (4, 3, n) in Julia's column-major order (permutedims of the usual 3x4), or (4, 3) for
# all scans.  Returns depth (w, h, n) on the device, 0 = no measurement; with return_counts also
# counts (2, n) = points stored, pixels hit.  At most LIDAR_MAX_SCANS scans per call.  No host sync.
const LIDAR_MAX_SCANS = 64
function lidar_depth(points::ROCArray{Float32,2}, offsets::Vector{Int64}, P::Array{Float32}, h, w;
                     forward_only=true, vel_depth=false, return_counts=false)
    size(points, 1) == 4 || error("points must be (4, M)")
    n = length(offsets) - 1
    1 <= n <= LIDAR_MAX_SCANS || error("1..", LIDAR_MAX_SCANS, " scans per call, got ", n)
    ndims(P) == 2 && (P = repeat(reshape(P, 4, 3, 1), 1, 1, n))
    size(P) == (4, 3, n) || error("P must be (4, 3) or (4, 3, ", n, ")")
    offsets[end] <= size(points, 2) || error("offsets end past the points")
    cfg = LidarCfg(n, h, w, forward_only ? 1 : 0, vel_depth ? 1 : 0)
    depth = ROCArray{Float32}(undef, w, h, n); counts = ROCArray{Int32}(undef, 2, n)
    check(ccall((:md2_lidar_depth, lib), Cint,
                (Ref{LidarCfg}, Ptr{Float32}, Ptr{Clonglong}, Ptr{Float32}, Ptr{Float32}, Ptr{Int32}, Ptr{Cvoid}),
                cfg, points, offsets, P, depth, counts, stream_ptr()))
    return return_counts ? (depth, counts) : depth
end

# Monodepth's flip post-processing ("+pp"): disp (w,h,n) or (w,h,1,n) blended with disp_flipped,
# the network's output for the horizontally mirrored frame as produced (not mirrored back).
function post_process_disparity(disp::ROCArray{Float32}, disp_flipped::ROCArray{Float32})
    (ndims(disp) == 3 || (ndims(disp) == 4 && size(disp, 3) == 1)) || error("disp must be (w,h,n) or (w,h,1,n)")
    size(disp) == size(disp_flipped) || error("disp_flipped must have disp's size")
    out = similar(disp)
    check(ccall((:md2_disp_post_process, lib), Cint,
                (Ptr{Float32}, Ptr{Float32}, Cint, Cint, Cint, Ptr{Float32}, Ptr{Cvoid}),
                disp, disp_flipped, size(disp, ndims(disp)), size(disp, 2), size(disp, 1), out, stream_ptr()))
    return out
end

# Frame resize on the device (include/md2.h states every operation of both filters): src holds the
# decoded images, image i the src_h[i] rows of src_w[i] interleaved c-byte pixels that start at the
# 0-based byte offsets[i].  Returns the planes (w, h, c, m) as Float32 -- m = 3n frames in order is
# the batch (w, h, c, 3, n) -- with return_u8 also the N0f8 bytes.  filter = RESIZE_IMRESIZE gives
# the host loader's bytes, RESIZE_ANTIALIAS the triangle filter widened by the reduction factor.
# At most RESIZE_MAX_IMAGES images per call.  No host sync.
const RESIZE_MAX_IMAGES = 64
const RESIZE_IMRESIZE = 0
const RESIZE_ANTIALIAS = 1
function resize_frames(src::ROCVector{UInt8}, offsets::Vector{Int64}, src_w::Vector{Int32}, src_h::Vector{Int32}, h, w;
                       channels, filter=RESIZE_IMRESIZE, quantize=true, flips=nothing, return_u8=false)
    m = length(offsets)
    1 <= m <= RESIZE_MAX_IMAGES || error("1..", RESIZE_MAX_IMAGES, " images per call, got ", m)
    length(src_w) == m && length(src_h) == m || error("one size per image: ", m)
    flips === nothing || length(flips) == m || error("one flip per image: ", m)
    all(offsets .>= 0) && all(offsets .+ Int64.(src_w) .* src_h .* channels .<= length(src)) ||
        error("every image must lie within src")
    (!return_u8 || quantize) || error("return_u8 needs quantize")
    cfg = ResizeCfg(m, channels, h, w, filter, quantize ? 1 : 0)
    out = ROCArray{Float32}(undef, w, h, channels, m)
    u8 = return_u8 ? ROCArray{UInt8}(undef, w, h, channels, m) : nothing
    fl = flips === nothing ? C_NULL : Vector{UInt8}(flips .!= 0)      # ccall keeps its arguments alive
    check(ccall((:md2_resize_frames, lib), Cint,
                (Ref{ResizeCfg}, Ptr{UInt8}, Ptr{Clonglong}, Ptr{Cint}, Ptr{Cint}, Ptr{UInt8}, Ptr{Float32}, Ptr{UInt8},
                 Ptr{Cvoid}),
                cfg, src, offsets, src_w, src_h, fl, out, u8 === nothing ? C_NULL : u8, stream_ptr()))
    return return_u8 ? (out, u8) : out
end

# Colour augmentation (torchvision's ColorJitter; include/md2.h states every operation): x
# (w,h,c,frames,n) with c = 1 or 3, params one Jitter per sample (factors, the order of the four
# operations as 0 brightness, 1 contrast, 2 saturation, 3 hue, and apply = 0 to copy the sample).
# Returns the jittered frames -- the x_net of train_loss; with return_means also the (frames, n)
# contrast means.  out may be x (in place).  At most JITTER_MAX_SAMPLES samples per call.  No host sync.
const JITTER_MAX_SAMPLES = 64
function color_jitter(x::ROCArray{Float32,5}, params::Vector{Jitter}; out=similar(x), return_means=false)
    w, h, c, frames, n = size(x)
    length(params) == n || error("one Jitter per sample: ", n, ", got ", length(params))
    1 <= n <= JITTER_MAX_SAMPLES || error("1..", JITTER_MAX_SAMPLES, " samples per call, got ", n)
    size(out) == size(x) || error("out must have x's size")
    ws = ROCVector{Float64}(undef, cld(ccall((:md2_color_jitter_workspace_size, lib), Csize_t,
                                             (Cint, Cint, Cint, Cint), n, frames, h, w), 8))
    means = ROCArray{Float32}(undef, frames, n)
    check(ccall((:md2_color_jitter, lib), Cint,
                (Ptr{Float32}, Cint, Cint, Cint, Cint, Cint, Ptr{Jitter}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid},
                 Ptr{Cvoid}),
                x, n, frames, c, h, w, params, out, means, ws, stream_ptr()))
    return return_means ? (out, means) : out
end

# Odometry evaluation (Monodepth2's snippet ATE; include/md2.h states every operation): pred (6, M)
# raw (rvec, tvec) steps, gt_rel (12, M) ground-truth steps (R row-major, t), offsets: nseq+1 0-based
# host offsets from 0 to M splitting the steps into sequences.  Returns device arrays per_snippet
# (3, S) = ate, scale, rot_chord, summary (4, nseq) = mean_ate, std_ate, mean_scale, mean_rot_chord
# and counts (2, nseq) = snippets, n_bad; with return_rt also the step transforms (12, M).
# invert=true inverts every predicted step first (eval_pose outputs against inv(G_k) G_{k+1}).
# At most POSE_EVAL_MAX_SEQ sequences per call.  No host sync.
const POSE_EVAL_MAX_SEQ = 64
function pose_errors(pred::ROCArray{Float32,2}, gt_rel::ROCArray{Float32,2};
                     offsets::Vector{Int64}=Int64[0, size(pred, 2)], track_length=5, invert=true, return_rt=false)
    size(pred, 1) == 6 || error("pred must be (6, M)")
    M = size(pred, 2)
    size(gt_rel) == (12, M) || error("gt_rel must be (12, ", M, ")")
    nseq = length(offsets) - 1
    1 <= nseq <= POSE_EVAL_MAX_SEQ || error("1..", POSE_EVAL_MAX_SEQ, " sequences per call, got ", nseq)
    (offsets[1] == 0 && offsets[end] == M) || error("offsets must run from 0 to the number of steps")
    S = sum(max(offsets[i + 1] - offsets[i] - track_length + 2, 0) for i in 1:nseq)
    out = ROCArray{Float32}(undef, 3, S); summary = ROCArray{Float32}(undef, 4, nseq)
    counts = ROCArray{Int32}(undef, 2, nseq); rt = ROCArray{Float32}(undef, 12, M)
    ws = ROCVector{UInt8}(undef, max(ccall((:md2_pose_eval_workspace_size, lib), Csize_t, (Clonglong,), M), 256))
    check(ccall((:md2_pose_eval, lib), Cint,
                (Ptr{Float32}, Ptr{Float32}, Ptr{Clonglong}, Cint, Cint, Cint, Ptr{Float32}, Ptr{Float32},
                 Ptr{Int32}, Ptr{Float32}, Ptr{UInt8}, Ptr{Cvoid}),
                pred, gt_rel, offsets, nseq, track_length, invert ? 1 : 0, out, summary, counts, rt, ws,
                stream_ptr()))
    return return_rt ? (out, summary, counts, rt) : (out, summary, counts)
end

function find_static(dataset, α; batch=16)
    keep = String[]
    for b0 in 1:batch:length(dataset)
        idx = b0:min(length(dataset), b0 + batch - 1)
        x = ROCArray(cat([dataset[i] for i in idx]...; dims=5))
        s = static_scores(x; target_id=dataset.target_id, source_ids=dataset.source_ids)
        append!(keep, dataset.files[idx][s .> α])
    end
    return keep
end

# One whole step (forward, loss, backward, ADAM(η) with β = (0.9, 0.999), ϵ = 1e-8) replayed as a
# captured hipGraph; the same kernels in the same order as train_loss + gradient! + update!
# the captured step with stereo supervision (md2_model_train_step_graph_stereo; see train_loss_stereo)
function train_step_graph_stereo!(m::HIPModel, x::ROCArray{Float32,5}, x_stereo::ROCArray{Float32,4},
                                  stereo_Rt::ROCArray{Float32,2}, auto_loss, η; temporal::Bool=true, x_net=nothing)
    m.packed || repack!(m)
    m.step += 1; loss = ROCVector{Float32}(undef, 1)
    check(ccall((:md2_model_train_step_graph_stereo, lib), Cint,
                (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cint, Ptr{Float32},
                 Ptr{Float32}, Ptr{Float32}, Cfloat, Cint, Ptr{Float32}, Ptr{Cvoid}),
                m.handle, x, ptr(x_net), x_stereo, stereo_Rt, temporal ? 1 : 0, ptr(auto_loss), m.m, m.v, η,
                m.step, loss, stream_ptr()))
    return loss
end

function train_step_graph!(m::HIPModel, x::ROCArray{Float32,5}, auto_loss, η; x_net=nothing)
    m.packed || repack!(m)
    m.step += 1; loss = ROCVector{Float32}(undef, 1)
    if x_net === nothing
        check(ccall((:md2_model_train_step_graph, lib), Cint,
                    (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Cint,
                     Ptr{Float32}, Ptr{Cvoid}),
                    m.handle, x, ptr(auto_loss), m.m, m.v, η, m.step, loss, stream_ptr()))
    else
        check(ccall((:md2_model_train_step_graph_aug, lib), Cint,
                    (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cfloat, Cint,
                     Ptr{Float32}, Ptr{Cvoid}),
                    m.handle, x, x_net, ptr(auto_loss), m.m, m.v, η, m.step, loss, stream_ptr()))
    end
    return loss
end

# ------------------------------------------------------------------------------------------------
# MINE plane rendering of the MPI mode (src/render.jl:21-114), forward only as upstream.  Same
# names and argument order as the reference; `pose` is a Pose(rvec (3,B), tvec (3,B)) and goes to
# the library as (6,B) = [B][6]; K / invK are host 3x3 matrices.
# ------------------------------------------------------------------------------------------------
pose6(pose) = ROCArray{Float32}(vcat(reshape(pose.rvec, 3, :), reshape(pose.tvec, 3, :)))

function get_src_xyz_from_plane_disparity(meshgrid_src_homo, mpi_disparity_src::ROCArray{Float32,2}, K_src_inv)
    _, W, H = size(meshgrid_src_homo)                  # create_meshgrid(H, W): the kernel's grid
    N, B = size(mpi_disparity_src); xyz = ROCArray{Float32}(undef, 3, W, H, N, B)
    iK = collect(rowmajor(K_src_inv))
    check(ccall((:md2_mine_src_xyz, lib), Cint,
                (Ptr{Float32}, Cint, Cint, Cint, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
                mpi_disparity_src, N, B, H, W, iK, xyz, stream_ptr()))
    return xyz
end

function get_tgt_xyz_from_plane_disparity(xyz_src::ROCArray{Float32,5}, pose)
    _, W, H, N, B = size(xyz_src); out = similar(xyz_src)
    check(ccall((:md2_mine_tgt_xyz, lib), Cint,
                (Ptr{Float32}, Ptr{Float32}, Cint, Cint, Cint, Cint, Ptr{Float32}, Ptr{Cvoid}),
                xyz_src, pose6(pose), N, B, H, W, out, stream_ptr()))
    return out
end

# sample(src (W,H,C,N*B), depth_src (N,B), pose, K, K_inv) -> (tgt, valid_mask (W*H, N*B))
function sample(src::ROCArray{Float32,4}, depth_src::ROCArray{Float32,2}, pose, K, K_inv)
    W, H, C, NB = size(src); N, B = size(depth_src)
    tgt = similar(src); valid = ROCArray{Float32}(undef, W * H, NB)
    k = collect(rowmajor(K)); ik = collect(rowmajor(K_inv))
    check(ccall((:md2_mine_sample, lib), Cint,
                (Ptr{Float32}, Cint, Ptr{Float32}, Ptr{Float32}, Cint, Cint, Cint, Cint, Ptr{Float32},
                 Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
                src, C, depth_src, pose6(pose), N, B, H, W, k, ik, tgt, valid, stream_ptr()))
    return tgt, valid .> 0
end

function plane_volume_rendering(rgb::ROCArray{Float32,5}, sigma::ROCArray{Float32,5}, xyz::ROCArray{Float32,5})
    W, H, _, N, B = size(rgb)
    rgb_out = ROCArray{Float32}(undef, W, H, 3, B)
    acc = ROCArray{Float32}(undef, W, H, 1, N, B); weights = similar(acc)
    check(ccall((:md2_plane_volume_rendering, lib), Cint,
                (Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Cint, Cint, Cint, Cint, Ptr{Float32},
                 Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
                rgb, sigma, xyz, N, B, H, W, rgb_out, acc, weights, stream_ptr()))
    return rgb_out, acc, weights
end

# one fused kernel: homography warp of rgb/sigma/xyz per plane + volume rendering + valid count
function render_tgt_rgb_depth(rgb::ROCArray{Float32,5}, sigma::ROCArray{Float32,5},
                              disparity_src::ROCArray{Float32,2}, xyz_tgt::ROCArray{Float32,5}, pose, K_inv, K)
    W, H, _, N, B = size(rgb)
    rgb_out = ROCArray{Float32}(undef, W, H, 3, B)
    depth = ROCArray{Float32}(undef, W, H, 1, N, B); mask = ROCArray{Float32}(undef, W, H, 1, 1, B)
    ik = collect(rowmajor(K_inv)); k = collect(rowmajor(K))
    check(ccall((:md2_render_tgt_rgb_depth, lib), Cint,
                (Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32},
                 Ptr{Float32}, Cint, Cint, Cint, Cint, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
                rgb, sigma, disparity_src, xyz_tgt, pose6(pose), ik, k, N, B, H, W, rgb_out, depth, mask,
                stream_ptr()))
    return rgb_out, depth, mask
end

# ------------------------------------------------------------------------------------------------
# Data parallel: one Julia process per GPU over the library's own RCCL communicator (SURVEY 8e;
# the reference's loop is scripts/script.jl:84-86).  Rank 0 writes the unique id to `idfile`,
# tagged with `run_id` -- a string unique to this launch that every rank gets from the launcher
# (e.g. the job id) -- and the other ranks accept only a file carrying their own tag, so a file
# left over from an earlier run can never hand them a stale id (ncclCommInitRank would hang).
# ------------------------------------------------------------------------------------------------
function comm_init(rank, nranks, device, idfile; run_id=get(ENV, "MD2_RUN_ID", ""), timeout_s=300)
    isempty(run_id) && error("comm_init: pass run_id (or set MD2_RUN_ID) unique to this launch")
    tag = Vector{UInt8}(run_id)
    id = zeros(UInt8, 128)
    if rank == 0
        check(ccall((:md2_comm_get_unique_id, lib), Cint, (Ptr{UInt8},), id))
        write(idfile * ".tmp", vcat(id, tag)); mv(idfile * ".tmp", idfile; force=true)
    else
        t0 = time()
        while true
            if isfile(idfile)
                b = read(idfile)
                if length(b) == 128 + length(tag) && b[129:end] == tag
                    id .= b[1:128]
                    break
                end
            end
            time() - t0 > timeout_s && error("comm_init: rank ", rank, " saw no id file ", idfile,
                                             " tagged ", run_id, " from rank 0 within ", timeout_s, " s")
            sleep(0.05)
        end
    end
    c = Ref{Ptr{Cvoid}}()
    check(ccall((:md2_comm_init, lib), Cint, (Cint, Cint, Ptr{UInt8}, Cint, Ref{Ptr{Cvoid}}),
                rank, nranks, id, device, c))
    return c[]
end

# forward + loss + backward with each bucket's RCCL all-reduce overlapped + ADAM (1/nranks)
function train_step_dp!(m::HIPModel, comm::Ptr{Cvoid}, x, auto_loss, η; β=(0.9f0, 0.999f0), ϵ=1f-8)
    m.packed || repack!(m)
    m.step += 1; loss = ROCVector{Float32}(undef, 1)
    check(ccall((:md2_model_train_step_dp, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32},
                 Cfloat, Cfloat, Cfloat, Cfloat, Cint, Ptr{Float32}, Ptr{Cvoid}),
                m.handle, comm, x, ptr(auto_loss), m.m, m.v, η, β[1], β[2], ϵ, m.step, loss, stream_ptr()))
    return loss
end

# MPI mode: the disparity bins of the next train_loss, [batch][num_bins] on the device -- the
# uniformly_sample_disparity_from_linspace_bins draw of src/model.jl:17-21 (CUDA.rand there)
function set_disparity_bins!(m::HIPModel, bins::ROCArray{Float32,2})
    check(ccall((:md2_model_set_disparity_bins, lib), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Cvoid}),
                m.handle, bins, stream_ptr()))
    return m
end

# Per-sample intrinsics of every following train_loss / train_step (plain, _aug, _stereo, graph, dp):
# K, invK (9, batch) each, column i = sample i's 3x3 in row-major order (vec(K_i')), copied into
# executor-owned buffers.  set_intrinsics!(m) returns to the ModelCfg's K.  The captured step is
# captured again when intrinsics come or go, not when their values change.  Not in MPI mode.
function set_intrinsics!(m::HIPModel, K::ROCArray{Float32,2}, invK::ROCArray{Float32,2})
    (size(K) == (9, m.cfg.batch) && size(invK) == (9, m.cfg.batch)) ||
        error("K and invK must be (9, batch) = ", (9, m.cfg.batch))
    check(ccall((:md2_model_set_intrinsics, lib), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
                m.handle, K, invK, stream_ptr()))
    return m
end
function set_intrinsics!(m::HIPModel)
    check(ccall((:md2_model_set_intrinsics, lib), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
                m.handle, C_NULL, C_NULL, stream_ptr()))
    return m
end

# ------------------------------------------------------------------------------------------------
# Data path (src/dtk.jl:29-46 Depth10k + FlipX, src/kitty.jl:45-61 KittyDataset): PNGs decoded on
# the host's cores into N0f8 bytes, widened to Float32 on the GPU
# ------------------------------------------------------------------------------------------------
function png_size(path::AbstractString)
    w, h, c = Ref{Cint}(0), Ref{Cint}(0), Ref{Cint}(0)
    check(ccall((:md2_png_info, lib), Cint, (Cstring, Ref{Cint}, Ref{Cint}, Ref{Cint}), path, w, h, c))
    return (w[], h[], c[])
end

function _to_device(bytes::Vector{UInt8}, dims)
    d8 = ROCArray(bytes)
    out = ROCArray{Float32}(undef, dims...)
    check(ccall((:md2_unorm8_to_float, lib), Cint, (Ptr{UInt8}, Ptr{Float32}, Clonglong, Ptr{Cvoid}),
                d8, out, length(bytes), stream_ptr()))
    return out
end

# Depth10k triplets (3W x H side-by-side RGB PNGs) -> x::(W, H, 3, 3, n) Float32 on the device
function load_triplets(paths::Vector{String}, width, height; flip=falses(length(paths)), threads=Threads.nthreads())
    n = length(paths)
    buf = Vector{UInt8}(undef, n * 3 * 3 * height * width)
    fl = UInt8.(flip)
    check(ccall((:md2_load_triplets_u8, lib), Cint,
                (Ptr{Cstring}, Cint, Cint, Cint, Ptr{UInt8}, Ptr{UInt8}, Cint),
                paths, n, width, height, fl, buf, threads))
    return _to_device(buf, (width, height, 3, 3, n))
end

# KittyDataset: paths[3i+k] = frame k of sample i (8-bit gray), imresize'd to (height, width)
function load_kitti(paths::Vector{String}, height, width; flip=falses(length(paths) ÷ 3), threads=Threads.nthreads())
    n = length(paths) ÷ 3
    buf = Vector{UInt8}(undef, n * 3 * height * width)
    fl = UInt8.(flip)
    check(ccall((:md2_load_kitti_u8, lib), Cint,
                (Ptr{Cstring}, Cint, Cint, Cint, Ptr{UInt8}, Ptr{UInt8}, Cint),
                paths, n, height, width, fl, buf, threads))
    return _to_device(buf, (width, height, 1, 3, n))
end

end # module
