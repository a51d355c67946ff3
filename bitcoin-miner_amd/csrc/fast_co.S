/* fast_co.S -- embeds the fast_search code object (fast_search.hip after the
   issue-priority pass, built by the Makefile into build/fast_search.hsaco) in
   libminehip.so.  search_kernels.hip loads it per device (hipModuleLoadData).
   Next to it, as a blob of its own, the first-hit kernels of mh_search_first
   (the same source with -DMH_FIRST through the same passes,
   build/fast_first.hsaco), loaded per device by the first mh_search_first,
   and the hits kernels of mh_search_hits (-DMH_HITS, build/fast_hits.hsaco),
   loaded per device by the first mh_search_hits, and the batch kernels of
   mh_search_batch_ex (-DMH_BATCH, build/fast_batch.hsaco), loaded per device
   by the first such call that fuses a fast piece, and the first-hit batch
   kernels of mh_search_first_batch_ex (-DMH_BATCH -DMH_FIRST,
   build/fast_batch_first.hsaco), loaded likewise, and the hits batch kernels
   of mh_search_hits_batch_ex (-DMH_BATCH -DMH_HITS,
   build/fast_batch_hits.hsaco), loaded likewise, and the stopping first-hit
   kernels of mh_search_first_ex (-DMH_FIRST -DMH_STOP,
   build/fast_first_stop.hsaco), loaded per device by the first such search
   that asks for MH_FIRST_STOP_RUNNING, and the stopping first-hit batch
   kernels of mh_search_first_batch_stop (-DMH_BATCH -DMH_FIRST -DMH_STOP,
   build/fast_batch_first_stop.hsaco), loaded per device by the first such
   call that fuses a fast piece, and the stopping hits kernels of
   mh_search_first_hits (-DMH_HITS -DMH_STOP, build/fast_hits_stop.hsaco),
   loaded per device by the first such call, and the stopping hits batch
   kernels of mh_search_first_hits_batch (-DMH_BATCH -DMH_HITS -DMH_STOP,
   build/fast_batch_bound.hsaco), loaded per device by the first such call
   that fuses a fast piece. */
    .section .rodata
    .p2align 12
    .globl mh_fast_co_begin
    .type mh_fast_co_begin, @object
mh_fast_co_begin:
    .incbin "fast_search.hsaco"
    .globl mh_fast_co_end
mh_fast_co_end:
    .size mh_fast_co_begin, mh_fast_co_end - mh_fast_co_begin
    .p2align 12
    .globl mh_first_co_begin
    .type mh_first_co_begin, @object
mh_first_co_begin:
    .incbin "fast_first.hsaco"
    .globl mh_first_co_end
mh_first_co_end:
    .size mh_first_co_begin, mh_first_co_end - mh_first_co_begin
    .p2align 12
    .globl mh_hits_co_begin
    .type mh_hits_co_begin, @object
mh_hits_co_begin:
    .incbin "fast_hits.hsaco"
    .globl mh_hits_co_end
mh_hits_co_end:
    .size mh_hits_co_begin, mh_hits_co_end - mh_hits_co_begin
    .p2align 12
    .globl mh_batch_co_begin
    .type mh_batch_co_begin, @object
mh_batch_co_begin:
    .incbin "fast_batch.hsaco"
    .globl mh_batch_co_end
mh_batch_co_end:
    .size mh_batch_co_begin, mh_batch_co_end - mh_batch_co_begin
    .p2align 12
    .globl mh_batch_first_co_begin
    .type mh_batch_first_co_begin, @object
mh_batch_first_co_begin:
    .incbin "fast_batch_first.hsaco"
    .globl mh_batch_first_co_end
mh_batch_first_co_end:
    .size mh_batch_first_co_begin, mh_batch_first_co_end - mh_batch_first_co_begin
    .p2align 12
    .globl mh_batch_hits_co_begin
    .type mh_batch_hits_co_begin, @object
mh_batch_hits_co_begin:
    .incbin "fast_batch_hits.hsaco"
    .globl mh_batch_hits_co_end
mh_batch_hits_co_end:
    .size mh_batch_hits_co_begin, mh_batch_hits_co_end - mh_batch_hits_co_begin
    .p2align 12
    .globl mh_first_stop_co_begin
    .type mh_first_stop_co_begin, @object
mh_first_stop_co_begin:
    .incbin "fast_first_stop.hsaco"
    .globl mh_first_stop_co_end
mh_first_stop_co_end:
    .size mh_first_stop_co_begin, mh_first_stop_co_end - mh_first_stop_co_begin
    .p2align 12
    .globl mh_batch_first_stop_co_begin
    .type mh_batch_first_stop_co_begin, @object
mh_batch_first_stop_co_begin:
    .incbin "fast_batch_first_stop.hsaco"
    .globl mh_batch_first_stop_co_end
mh_batch_first_stop_co_end:
    .size mh_batch_first_stop_co_begin, mh_batch_first_stop_co_end - mh_batch_first_stop_co_begin
    .p2align 12
    .globl mh_hits_stop_co_begin
    .type mh_hits_stop_co_begin, @object
mh_hits_stop_co_begin:
    .incbin "fast_hits_stop.hsaco"
    .globl mh_hits_stop_co_end
mh_hits_stop_co_end:
    .size mh_hits_stop_co_begin, mh_hits_stop_co_end - mh_hits_stop_co_begin
    .p2align 12
    .globl mh_batch_bound_co_begin
    .type mh_batch_bound_co_begin, @object
mh_batch_bound_co_begin:
    .incbin "fast_batch_bound.hsaco"
    .globl mh_batch_bound_co_end
mh_batch_bound_co_end:
    .size mh_batch_bound_co_begin, mh_batch_bound_co_end - mh_batch_bound_co_begin
    .section .note.GNU-stack,"",@progbits
