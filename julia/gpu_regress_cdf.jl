# gpu_regress_cdf.jl -- include/dpmm_hip_regress_cdf.h from Julia: the conditional CDF and the quantiles of every target given the features
# a GpuWorker holds, after set_regression! (gpu_regress_draw.jl).  `include` behind gpu_worker.jl and gpu_regress_draw.jl (GpuWorker,
# dpmm_check, libdpmm).  Optional: nothing of the drop-in surface needs it.
#
# UNEXECUTED: the build image has no Julia.  Written against DPMM_ABI_VERSION 3.
#
# Arrays are the caller's, in C (row-major) order -- Julia arrays with the LAST C index first: y, cdf, sf (D_t, n); z (L, K): z[q, k] the
# quantile of t_{df_k + D_o} at levels[q] (host/condition.py: student_t_ppf forms it); the quantiles (D_t, L, n).

# (cdf (D_t, n), sf (D_t, n), labels (n), skipped): P(target <= y) and P(target > y) of the worker's n points, in host memory
function regress_cdf(w::GpuWorker, y::Matrix{Float32})
    Dt = size(y, 1)
    @assert size(y, 2) == w.n
    cdf = Matrix{Float32}(undef, Dt, w.n); sf = Matrix{Float32}(undef, Dt, w.n)
    labels = Vector{Int64}(undef, w.n); skipped = zeros(Int64, 1)
    dpmm_check(ccall((:dpmm_regress_cdf_points, libdpmm), Cint,
                     (Ptr{Cvoid}, Ptr{Float32}, Int64, Ptr{Float32}, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Int64}),
                     w.h, y, Dt, cdf, sf, Dt, labels, skipped), w)
    return cdf, sf, labels, skipped[1]
end

# the same from and into device memory the caller owns (rows ldy / ld floats apart; d_sf and d_labels may be C_NULL)
function regress_cdf_device!(w::GpuWorker, d_y::Ptr{Float32}, ldy::Integer, d_cdf::Ptr{Float32}, d_sf::Ptr{Float32}, ld::Integer, d_labels::Ptr{Int64})
    skipped = zeros(Int64, 1)
    dpmm_check(ccall((:dpmm_regress_cdf_points_device, libdpmm), Cint,
                     (Ptr{Cvoid}, Ptr{Float32}, Int64, Ptr{Float32}, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Int64}),
                     w.h, d_y, ldy, d_cdf, d_sf, ld, d_labels, skipped), w)
    return skipped[1]
end

# after set_regression!: L strictly increasing levels inside (0, 1) and their Student-t quantiles per cluster
function set_regression_levels!(w::GpuWorker, levels::Vector{Float64}, z::Matrix{Float64})
    @assert size(z) == (length(levels), w.K) && issorted(levels; lt = <=) && all(0 .< levels .< 1)
    dpmm_check(ccall((:dpmm_set_regression_levels, libdpmm), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}), w.h, length(levels), levels, z), w)
    return length(levels)
end

# (values (D_t, L, n), labels (n), skipped): the y at which the conditional CDF of every target reaches every level, in host memory
function regress_quantiles(w::GpuWorker, Dt::Integer, L::Integer)
    values = Array{Float32,3}(undef, Dt, L, w.n); labels = Vector{Int64}(undef, w.n); skipped = zeros(Int64, 1)
    dpmm_check(ccall((:dpmm_regress_quantile_points, libdpmm), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Int64}),
                     w.h, values, Dt, labels, skipped), w)
    return values, labels, skipped[1]
end

function regress_quantiles_device!(w::GpuWorker, d_values::Ptr{Float32}, ld::Integer, d_labels::Ptr{Int64})
    skipped = zeros(Int64, 1)
    dpmm_check(ccall((:dpmm_regress_quantile_points_device, libdpmm), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int64, Ptr{Int64}, Ptr{Int64}),
                     w.h, d_values, ld, d_labels, skipped), w)
    return skipped[1]
end
