# gpu_holdout.jl -- include/dpmm_hip_holdout.h from Julia: the points a GpuWorker holds that lie below the floors of the served model,
# compacted on the GPU into device memory of the caller, after dpmm_set_predictive_niw.  `include` behind gpu_worker.jl (GpuWorker,
# dpmm_check, libdpmm).  Optional: nothing of the drop-in surface needs it.  NIW and dense points only.
#
# UNEXECUTED: the build image has no Julia.  Written against DPMM_ABI_VERSION 3.
struct DpmmHoldoutOut             # dpmm_holdout_out
    total::Ptr{Int64}; stored::Ptr{Int64}; skipped::Ptr{Int64}; incomplete::Ptr{Int64}; scored::Ptr{Int64}
end

# dst_points: device memory of cap * D Float32 (point-major), dst_index: of cap Int64; a floor that is `nothing` is not in use
holdout_begin!(w::GpuWorker, dst_points::Ptr{Float32}, dst_index::Ptr{Int64}, cap::Integer;
               min_logdens::Union{Nothing,Real}=nothing, min_tail::Union{Nothing,Real}=nothing) =
    dpmm_check(ccall((:dpmm_holdout_begin, libdpmm), Cint, (Ptr{Cvoid}, Cint, Cfloat, Cint, Cfloat, Ptr{Float32}, Ptr{Int64}, Int64),
                     w.h, min_logdens === nothing ? 0 : 1, min_logdens === nothing ? 0f0 : Float32(min_logdens),
                     min_tail === nothing ? 0 : 1, min_tail === nothing ? 0f0 : Float32(min_tail), dst_points, dst_index, cap), w)

# the points 0 .. n_valid - 1 of the current upload, global indices lo + i (0-based)
holdout_accumulate!(w::GpuWorker, lo::Integer, n_valid::Integer) =
    dpmm_check(ccall((:dpmm_holdout_accumulate, libdpmm), Cint, (Ptr{Cvoid}, Int64, Int64), w.h, lo, n_valid), w)

# (total, stored, skipped, incomplete, scored) as they stand; waits for the worker's stream
function holdout_read(w::GpuWorker)
    c = zeros(Int64, 5)
    GC.@preserve c begin
        out = Ref(DpmmHoldoutOut(pointer(c, 1), pointer(c, 2), pointer(c, 3), pointer(c, 4), pointer(c, 5)))
        dpmm_check(ccall((:dpmm_holdout_read, libdpmm), Cint, (Ptr{Cvoid}, Ref{DpmmHoldoutOut}), w.h, out), w)
    end
    return c[1], c[2], c[3], c[4], c[5]
end
