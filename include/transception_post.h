/*
 * transception_post.h -- connected-component post-processing of predicted label volumes, C ABI of libtransception_hip.so
 * (MI355X / gfx950; csrc/postprocess.hip).
 *
 * A header of its own: every entry of transception_hip.h names the reference call sites it replaces, and these replace none -- the
 * reference has no post-processing step.  Self-contained (no #include); the conventions are those of transception_hip.h: device
 * pointers owned by the caller, `stream` a hipStream_t passed as void*, nothing allocated, freed or synchronised, every call
 * asynchronous on `stream`.  An unmarked entry returns a status with the values of transception_hip.h: 0 (TC_OK), -1 (TC_ERR_ARG),
 * -2 (TC_ERR_LAUNCH); an entry marked TC_QUERY returns a value instead.
 *
 * Definition (one for the device and for evaluate.postprocess_host, which states it on scipy.ndimage.label):
 *   - lab is a uint8 label volume [D,H,W] ([H,W] is passed as D = 1).  A voxel is foreground if 1 <= lab[v] < ncls; label 0 and labels
 *     >= ncls are background, copied through unchanged, and never join a component;
 *   - two foreground voxels are in one component if they carry the same label and a chain of neighbours of that label links them.
 *     connectivity = 1: face neighbours (6; 4 when D = 1), scipy's generate_binary_structure(ndim, 1); connectivity = 3: the full
 *     neighbourhood (26; 8 when D = 1), generate_binary_structure(ndim, ndim);
 *   - the root of a component is the smallest linear index (z H + y) W + x among its voxels; its size is its voxel count;
 *   - the largest component of class k has the greatest size; a TIE goes to the SMALLER root (the component scipy.ndimage.label numbers
 *     first, which is what numpy.argmax over its sizes picks).
 * Integer work and integer atomics only, and every output is defined without reference to an order of arrival: bit-identical from run
 * to run.
 * Limits (-1 beyond them, as for null pointers; nothing is launched): D, H, W in 1..2048, D*H*W < 2^31, ncls in 2..16, connectivity 1
 * or 3, mode one of the two below, min_voxels >= 1 with TC_CC_MIN_VOXELS.
 *
 * tc_cc_scratch_bytes: what the three entries need beside lab and out: root and size, int32 [D,H,W] each = 8 bytes a voxel (0 for a shape
 *   outside the limits); best is 16 * ncls bytes more.
 * tc_cc_label: root[v] = root of v's component for foreground v, -1 for background; int32 [D,H,W], OVERWRITTEN (it is the union-find's
 *   parent array while the entry runs).  Three launches (init, merge, compress); no loop in any of them waits for another thread.
 * tc_cc_sizes: size[r] = voxel count of the component with root r, 0 at every voxel that is not a root; int32 [D,H,W], OVERWRITTEN.
 *   best[2k], best[2k+1] = (voxels, root) of the largest component of class k under the tie rule above, (0, -1) for a class without a
 *   voxel and for k = 0; int64 [ncls][2], OVERWRITTEN.  root is what tc_cc_label wrote for the same lab.
 * tc_cc_keep: out[v] = lab[v] for background v; for foreground v, mode TC_CC_LARGEST: lab[v] if root[v] == best[2 lab[v] + 1], else 0
 *   (min_voxels is not read); mode TC_CC_MIN_VOXELS: lab[v] if size[root[v]] >= min_voxels, else 0.  out is uint8 [D,H,W], OVERWRITTEN;
 *   out may be lab itself (each voxel is read and written by one thread only).
 */
#ifndef TRANSCEPTION_POST_H
#define TRANSCEPTION_POST_H

#ifdef __cplusplus
extern "C" {
#endif

#define TC_POST_ABI_VERSION 1
#ifndef TC_QUERY
#define TC_QUERY
#endif
enum { TC_CC_LARGEST = 0, TC_CC_MIN_VOXELS = 1 };

/* identity of this part of the library: bumped on any change to a signature below */
TC_QUERY int tc_post_abi_version(void);
TC_QUERY long long tc_cc_scratch_bytes(int D, int H, int W);
int tc_cc_label(const unsigned char* lab, int* root, int D, int H, int W, int ncls, int connectivity, void* stream);
int tc_cc_sizes(const unsigned char* lab, const int* root, int* size, long long* best, int D, int H, int W, int ncls, void* stream);
int tc_cc_keep(const unsigned char* lab, const int* root, const int* size, const long long* best, unsigned char* out, int mode,
               long long min_voxels, int D, int H, int W, int ncls, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRANSCEPTION_POST_H */
