# gpu_recommend.jl -- include/dpmm_hip_recommend.h from Julia: the m features a count point is expected to get next under a fitted
# Multinomial model, among those it does not hold yet.  `include` behind gpu_worker.jl (GpuWorker, dpmm_check, libdpmm), after the
# worker has its points and set_predictive_mult.  Optional: nothing of the drop-in surface needs it.
#
# UNEXECUTED: the build image has no Julia.  Written against DPMM_ABI_VERSION 3.
#
# Arrays are the caller's, in C (row-major) order -- Julia arrays with the LAST C index first: theta (D, K) with theta[d, k] =
# alpha'_kd / sum_d alpha'_kd in Float64; features and prob (m, n), features 0-BASED as the library writes them (-1: no candidate left).

const DPMM_RECOMMEND_MAX_TOP = 16

# theta for the predictive parameters in force; a later set_predictive_* invalidates it
function set_recommend!(w::GpuWorker, theta::Matrix{Float64})
    @assert size(theta) == (w.D, w.K)
    dpmm_check(ccall((:dpmm_set_recommend, libdpmm), Cint, (Ptr{Cvoid}, Ptr{Float64}), w.h, theta), w)
    return nothing
end

# (features (m, n) Int32, prob (m, n) Float32, labels (n), skipped) of the worker's n points, in host memory
function recommend(w::GpuWorker, m::Integer; exclude_seen::Bool = true)
    @assert 1 <= m <= min(w.D, DPMM_RECOMMEND_MAX_TOP)
    features = Matrix{Int32}(undef, m, w.n); prob = Matrix{Float32}(undef, m, w.n)
    labels = Vector{Int64}(undef, w.n); skipped = zeros(Int64, 1)
    dpmm_check(ccall((:dpmm_recommend_points, libdpmm), Cint,
                     (Ptr{Cvoid}, Cint, Cint, Ptr{Int32}, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Int64}),
                     w.h, m, exclude_seen ? 1 : 0, features, prob, m, labels, skipped), w)
    return features, prob, labels, skipped[1]
end

# the same into device memory the caller owns (rows ld words apart; d_labels may be C_NULL)
function recommend_device!(w::GpuWorker, m::Integer, d_features::Ptr{Int32}, d_prob::Ptr{Float32}, ld::Integer, d_labels::Ptr{Int64}; exclude_seen::Bool = true)
    skipped = zeros(Int64, 1)
    dpmm_check(ccall((:dpmm_recommend_points_device, libdpmm), Cint,
                     (Ptr{Cvoid}, Cint, Cint, Ptr{Int32}, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Int64}),
                     w.h, m, exclude_seen ? 1 : 0, d_features, d_prob, ld, d_labels, skipped), w)
    return skipped[1]
end
