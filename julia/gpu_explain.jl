# gpu_explain.jl -- include/dpmm_hip_explain.h from Julia: which features make a point atypical of its cluster, for every point a GpuWorker
# holds, after dpmm_set_predictive_niw.  `include` behind gpu_worker.jl (GpuWorker, dpmm_check, libdpmm).  Optional: nothing of the drop-in
# surface needs it.
#
# UNEXECUTED: the build image has no Julia.  Written against DPMM_ABI_VERSION 3.
struct DpmmExplainOut          # dpmm_explain_out
    labels::Ptr{Int64}; mahalanobis::Ptr{Float32}; tail::Ptr{Float32}; skipped::Ptr{Int64}; incomplete::Ptr{Int64}
    residual::Ptr{Float32}; zscore::Ptr{Float32}; feature_tail::Ptr{Float32}; features::Ptr{Int32}
    top::Int32; ld::Int64
end

# (labels, mahalanobis, tail, residual, zscore, feature_tail, features, skipped, incomplete) of the worker's n points, in host memory.
# top == 0: the three arrays are (D, n) in feature order -- the library's rows are point-major, which is Julia's column-major (D, n) -- and
# features is nothing.  top == m: they are (m, n), column i the m features of largest |zscore| of point i, and features (m, n) is 0-based.
function explain(w::GpuWorker, D::Integer; top::Integer = 0)
    ld = top == 0 ? Int(D) : Int(top)
    labels = Vector{Int64}(undef, w.n); q = Vector{Float32}(undef, w.n); tail = Vector{Float32}(undef, w.n)
    residual = Matrix{Float32}(undef, ld, w.n); zscore = Matrix{Float32}(undef, ld, w.n); ftail = Matrix{Float32}(undef, ld, w.n)
    features = top == 0 ? nothing : Matrix{Int32}(undef, ld, w.n)
    counters = zeros(Int64, 2)
    GC.@preserve labels q tail residual zscore ftail features counters begin
        out = Ref(DpmmExplainOut(pointer(labels), pointer(q), pointer(tail), pointer(counters, 1), pointer(counters, 2), pointer(residual),
                                 pointer(zscore), pointer(ftail), features === nothing ? Ptr{Int32}(C_NULL) : pointer(features), Int32(top), Int64(ld)))
        dpmm_check(ccall((:dpmm_explain_points, libdpmm), Cint, (Ptr{Cvoid}, Ref{DpmmExplainOut}), w.h, out), w)
    end
    return labels, q, tail, residual, zscore, ftail, features, counters[1], counters[2]
end
