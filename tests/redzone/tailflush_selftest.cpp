// Self-test of the tail-flush allocator (redzone_alloc.cpp, tf_malloc): the last 16 bytes of a tensor are readable on the GPU, the tensor
// ends exactly where its mapped memory ends, on a granule boundary, and a whole granule of the reservation behind it is left unmapped —
// the layout that makes a 16-byte read behind a tensor a GPU memory-access fault.  Nothing here reads outside a tensor.
//   hipcc -O2 -o tailflush_selftest tailflush_selftest.cpp redzone_alloc.cpp
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <sys/types.h>
extern "C" void* tf_malloc(ssize_t size, int device, hipStream_t stream);
extern "C" void tf_free(void* ptr, ssize_t size, int device, hipStream_t stream);
extern "C" long tf_sweep(void);
extern "C" size_t tf_granule(void);
extern "C" int tf_layout(const void* user, size_t* to_mapped_end, size_t* to_reserved_end);

__global__ void k_read16(const uint4* p, uint4* out) { out[0] = p[0]; }

int main() {
    const ssize_t size = 100000;        // not a multiple of anything interesting
    char* t = static_cast<char*>(tf_malloc(size, 0, nullptr));
    uint4* out = static_cast<uint4*>(tf_malloc(16, 0, nullptr));
    if (t == nullptr || out == nullptr) { printf("tf_malloc failed (virtual-memory API unavailable)\n"); return 3; }
    const size_t gran = tf_granule();
    printf("granule %zu bytes, tensor at %p\n", gran, (void*)t);
    const size_t used = ((size_t)size + 15) & ~(size_t)15;
    hipLaunchKernelGGL(k_read16, dim3(1), dim3(1), 0, 0, reinterpret_cast<const uint4*>(t + used - 16), out);
    if (hipDeviceSynchronize() != hipSuccess) { printf("the in-bounds read failed\n"); return 2; }
    printf("inside ok\n");
    size_t to_mapped = 0, to_reserved = 0;
    if (tf_layout(t, &to_mapped, &to_reserved) != 0) { printf("tf_layout does not know the tensor\n"); return 6; }
    const uintptr_t end = reinterpret_cast<uintptr_t>(t) + used;
    if (to_mapped != used || gran == 0 || end % gran != 0 || to_reserved < used + gran) {
        printf("not flush: %zu bytes to the end of the mapping, %zu to the end of the reservation, end %% granule = %zu\n", to_mapped,
               to_reserved, gran ? (size_t)(end % gran) : (size_t)0);
        return 7;
    }
    printf("flush ok: the tensor ends at a granule boundary, followed by %zu unmapped bytes of its reservation\n", to_reserved - used);
    tf_free(t, size, 0, nullptr); tf_free(out, 16, 0, nullptr);
    return tf_sweep() == 0 ? 0 : 5;
}
