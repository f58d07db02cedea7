# gpu_typicality.jl -- include/dpmm_hip_typicality.h from Julia: the calibrated outlier score of every point a GpuWorker holds, after
# dpmm_set_predictive_niw.  `include` behind gpu_worker.jl (GpuWorker, dpmm_check, libdpmm).  Optional: nothing of the drop-in surface
# needs it.
#
# UNEXECUTED: the build image has no Julia.  Written against DPMM_ABI_VERSION 3.
struct DpmmTypicalityOut          # dpmm_typicality_out
    labels::Ptr{Int64}; mahalanobis::Ptr{Float32}; tail::Ptr{Float32}; skipped::Ptr{Int64}; incomplete::Ptr{Int64}
end

# (labels, mahalanobis, tail, skipped, incomplete) of the worker's n points, in host memory
function typicality(w::GpuWorker)
    labels = Vector{Int64}(undef, w.n); q = Vector{Float32}(undef, w.n); tail = Vector{Float32}(undef, w.n)
    counters = zeros(Int64, 2)
    GC.@preserve labels q tail counters begin
        out = Ref(DpmmTypicalityOut(pointer(labels), pointer(q), pointer(tail), pointer(counters, 1), pointer(counters, 2)))
        dpmm_check(ccall((:dpmm_typicality_points, libdpmm), Cint, (Ptr{Cvoid}, Ref{DpmmTypicalityOut}), w.h, out), w)
    end
    return labels, q, tail, counters[1], counters[2]
end

# between dpmm_batchstats_begin and the first dpmm_batchstats_accumulate: complete points with a tail below min_tail are held out
set_min_tail!(w::GpuWorker, min_tail::Union{Nothing,Real}) =
    dpmm_check(ccall((:dpmm_batchstats_set_min_tail, libdpmm), Cint, (Ptr{Cvoid}, Cint, Cfloat),
                     w.h, min_tail === nothing ? 0 : 1, min_tail === nothing ? 0f0 : Float32(min_tail)), w)
