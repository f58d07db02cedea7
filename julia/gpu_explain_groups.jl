# gpu_explain_groups.jl -- include/dpmm_hip_explain_groups.h from Julia: which group of features makes a point atypical of its cluster, for
# every point a GpuWorker holds, after dpmm_set_predictive_niw.  `include` behind gpu_worker.jl (GpuWorker, dpmm_check, libdpmm).  Optional:
# nothing of the drop-in surface needs it.
#
# UNEXECUTED: the build image has no Julia.  Written against DPMM_ABI_VERSION 3.
using LinearAlgebra

struct DpmmExplainGroupsOut    # dpmm_explain_groups_out
    labels::Ptr{Int64}; mahalanobis::Ptr{Float32}; tail::Ptr{Float32}; skipped::Ptr{Int64}; incomplete::Ptr{Int64}
    group_mahalanobis::Ptr{Float32}; group_tail::Ptr{Float32}
    ld::Int64
end

# The tables of the header from the Float32 factors R (D, D, K), R[:, :, k] upper triangular with Sigma_k^-1 = R' R, widened: for every
# cluster and group A_GG = L L' and W = L^-1, packed per cluster, group after group, the rows of the lower triangle one after the other.
# groups: vectors of 1-BASED feature indices, increasing; the library is handed them 0-based.
function set_explain_groups(w::GpuWorker, R::Array{Float32,3}, groups::Vector{Vector{Int}})
    K = size(R, 3)
    W = Float64[]
    for k in 1:K
        Rk = UpperTriangular(Float64.(R[:, :, k]))
        A = Matrix(Rk' * Rk)
        for g in groups
            Li = inv(cholesky(Symmetric(A[g, g])).L)
            for r in 1:length(g), c in 1:r
                push!(W, Li[r, c])
            end
        end
    end
    offsets = Int64[0; cumsum(length.(groups))]
    features = Int32[f - 1 for g in groups for f in g]
    GC.@preserve offsets features W begin
        dpmm_check(ccall((:dpmm_set_explain_groups, libdpmm), Cint, (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}),
                         w.h, Int32(length(groups)), pointer(offsets), pointer(features), pointer(W)), w)
    end
    return nothing
end

# (labels, mahalanobis, tail, group_mahalanobis, group_tail, skipped, incomplete) of the worker's n points, in host memory.  The two
# arrays are (G, n): the library's rows are point-major, which is Julia's column-major (G, n).
function explain_groups(w::GpuWorker, G::Integer)
    labels = Vector{Int64}(undef, w.n); q = Vector{Float32}(undef, w.n); tail = Vector{Float32}(undef, w.n)
    gq = Matrix{Float32}(undef, G, w.n); gtail = Matrix{Float32}(undef, G, w.n)
    counters = zeros(Int64, 2)
    GC.@preserve labels q tail gq gtail counters begin
        out = Ref(DpmmExplainGroupsOut(pointer(labels), pointer(q), pointer(tail), pointer(counters, 1), pointer(counters, 2), pointer(gq),
                                       pointer(gtail), Int64(G)))
        dpmm_check(ccall((:dpmm_explain_groups_points, libdpmm), Cint, (Ptr{Cvoid}, Ref{DpmmExplainGroupsOut}), w.h, out), w)
    end
    return labels, q, tail, gq, gtail, counters[1], counters[2]
end
