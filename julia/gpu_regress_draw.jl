# gpu_regress_draw.jl -- include/dpmm_hip_regress.h and include/dpmm_hip_regress_draw.h from Julia: mixture regression from the features a
# GpuWorker holds (the GIVEN features: its D is D_o) to D_t targets, and draws of the targets from their conditional law, after
# dpmm_set_predictive_niw.  `include` behind gpu_worker.jl (GpuWorker, dpmm_check, libdpmm).  Optional: nothing of the drop-in surface
# needs it.
#
# UNEXECUTED: the build image has no Julia.  Written against DPMM_ABI_VERSION 3.
#
# The tables are the caller's, in Float64 and in C (row-major) order -- Julia arrays with the LAST C index first:
#   B (D_o, D_t, K): B[e, d, k] = B_k[d][e];  c, V (D_t, K);  h (K);  W (D_t, D_t, K): W[a, d, k] = W_k[d][a], W_k upper triangular,
#   W_k W_k' = (A_MM)^-1 (host/condition.py forms all five).

function set_regression!(w::GpuWorker, B::Array{Float64,3}, c::Matrix{Float64}, V::Matrix{Float64}, h::Vector{Float64})
    Dt = size(c, 1)
    @assert size(B) == (w.D, Dt, w.K) && size(c) == (Dt, w.K) && size(V) == (Dt, w.K) && length(h) == w.K
    dpmm_check(ccall((:dpmm_set_regression, libdpmm), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                     w.h, Dt, B, c, V, h), w)
    return Dt
end

# after set_regression!: the factor the draws multiply their normals with
function set_regression_factor!(w::GpuWorker, W::Array{Float64,3})
    @assert size(W, 1) == size(W, 2) && size(W, 3) == w.K
    dpmm_check(ccall((:dpmm_set_regression_factor, libdpmm), Cint, (Ptr{Cvoid}, Ptr{Float64}), w.h, W), w)
end

# (mean (D_t, n), std (D_t, n) or nothing, labels (n), skipped) of the worker's n points, in host memory
function regress(w::GpuWorker, Dt::Integer; std::Bool = false)
    mean = Matrix{Float32}(undef, Dt, w.n); sd = std ? Matrix{Float32}(undef, Dt, w.n) : nothing
    labels = Vector{Int64}(undef, w.n); skipped = zeros(Int64, 1)
    dpmm_check(ccall((:dpmm_regress_points, libdpmm), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Int64}),
                     w.h, mean, std ? sd : C_NULL, Dt, labels, skipped), w)
    return mean, sd, labels, skipped[1]
end

# (values (D_t, n, ndraws), components (n, ndraws) 0-based, -1: the point took no part, skipped): the draws draw0 .. draw0 + ndraws - 1 of the
# worker's n points, whose global indices are i0 .. i0 + n - 1, in host memory -- the stacked layout (ld = D_t, draw_stride = n D_t).
# A value depends on (seed, global index, draw index, the point, the model) alone.
function regress_draws(w::GpuWorker, Dt::Integer, ndraws::Integer; seed::Integer = 0, i0::Integer = 0, draw0::Integer = 0)
    values = Array{Float32,3}(undef, Dt, w.n, ndraws); comp = Matrix{Int32}(undef, w.n, ndraws); skipped = zeros(Int64, 1)
    dpmm_check(ccall((:dpmm_regress_draw_points, libdpmm), Cint,
                     (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, UInt64, Int64, Int64, Int64, Ptr{Int64}),
                     w.h, values, Dt, Int64(Dt) * w.n, comp, UInt64(seed), i0, draw0, ndraws, skipped), w)
    return values, comp, skipped[1]
end

# the same into device memory the caller owns (d_values: ndraws images of (n, ld) Float32 rows, draw_stride floats apart; d_comp: C_NULL or
# (ndraws, n) Int32), e.g. the pointers of AMDGPU.jl arrays
function regress_draws_device!(w::GpuWorker, d_values::Ptr{Float32}, ld::Integer, draw_stride::Integer, d_comp::Ptr{Int32}, ndraws::Integer;
                               seed::Integer = 0, i0::Integer = 0, draw0::Integer = 0)
    skipped = zeros(Int64, 1)
    dpmm_check(ccall((:dpmm_regress_draw_points_device, libdpmm), Cint,
                     (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, UInt64, Int64, Int64, Int64, Ptr{Int64}),
                     w.h, d_values, ld, draw_stride, d_comp, UInt64(seed), i0, draw0, ndraws, skipped), w)
    return skipped[1]
end
