# gpu_count_explain.jl -- include/dpmm_hip_count_explain.h from Julia: the features that put a count point out of the cluster a fitted
# Multinomial model gives it, with their binomial deviance residuals and exact one-sided tails.  `include` behind gpu_worker.jl (GpuWorker,
# dpmm_check, libdpmm), after the worker has its points and set_predictive_mult.  Optional: nothing of the drop-in surface needs it.
#
# UNEXECUTED: the build image has no Julia.  Written against DPMM_ABI_VERSION 3.
#
# Arrays are the caller's, in C (row-major) order -- Julia arrays with the LAST C index first: log_theta, log1m_theta and order (D, K);
# features, count, expected, residual, feature_tail (top, n), features 0-BASED as the library writes them (-1: no candidate left), and so
# is `order` (0-based feature indices).

const DPMM_COUNT_EXPLAIN_MAX_TOP = 16
const DPMM_COUNT_EXPLAIN_SIDES = Dict(:both => 0, :over => 1, :under => 2)

# mirrors dpmm_count_explain_out
struct CountExplainOut
    top::Cint
    side::Cint
    ld::Int64
    features::Ptr{Int32}
    count::Ptr{Float32}
    expected::Ptr{Float32}
    residual::Ptr{Float32}
    feature_tail::Ptr{Float32}
    labels::Ptr{Int64}
    total::Ptr{Float64}
    skipped::Ptr{Int64}
    incomplete::Ptr{Int64}
end

# the three tables from alpha' (D, K), for the predictive parameters in force; a later set_predictive_* invalidates them
function set_count_explain!(w::GpuWorker, alpha::Matrix{Float64})
    @assert size(alpha) == (w.D, w.K)
    theta = alpha ./ sum(alpha, dims = 1)
    lth = log.(theta); l1m = log1p.(-theta)
    order = Matrix{Int32}(undef, w.D, w.K)
    for k in 1:w.K
        order[:, k] = Int32.(sortperm(l1m[:, k], alg = MergeSort) .- 1)      # stable: equal values in increasing index order
    end
    dpmm_check(ccall((:dpmm_set_count_explain, libdpmm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), w.h, lth, l1m, order), w)
    return nothing
end

# (features, count, expected, residual, feature_tail (top, n), labels (n), total (n), skipped, incomplete) of the worker's n points, host memory
function count_explain(w::GpuWorker, top::Integer; side::Symbol = :both)
    @assert 1 <= top <= min(w.D, DPMM_COUNT_EXPLAIN_MAX_TOP)
    features = Matrix{Int32}(undef, top, w.n)
    count, expected, residual, tail = (Matrix{Float32}(undef, top, w.n) for _ in 1:4)
    labels = Vector{Int64}(undef, w.n); total = Vector{Float64}(undef, w.n); cnt = zeros(Int64, 2)
    GC.@preserve features count expected residual tail labels total cnt begin
        out = Ref(CountExplainOut(top, DPMM_COUNT_EXPLAIN_SIDES[side], top, pointer(features), pointer(count), pointer(expected), pointer(residual),
                                  pointer(tail), pointer(labels), pointer(total), pointer(cnt), pointer(cnt) + 8))
        dpmm_check(ccall((:dpmm_count_explain_points, libdpmm), Cint, (Ptr{Cvoid}, Ptr{CountExplainOut}), w.h, out), w)
    end
    return features, count, expected, residual, tail, labels, total, cnt[1], cnt[2]
end

# the same into device memory the caller owns (`out` filled with device addresses, rows ld words apart; skipped and incomplete stay host words)
function count_explain_device!(w::GpuWorker, out::Ref{CountExplainOut})
    dpmm_check(ccall((:dpmm_count_explain_points_device, libdpmm), Cint, (Ptr{Cvoid}, Ptr{CountExplainOut}), w.h, out), w)
    return nothing
end
