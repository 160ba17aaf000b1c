/*
 * fx.h — C-ABI of the MI355X-native per-scan detector/descriptor hot path.
 *
 * The reference (GAVLab/feature_extraction) has no plugin/FFI boundary; its hot
 * path is the body of FeatureExtractionNode::cloudCallback between message
 * conversion and the first publish (ref: src/feature_extraction_node.cpp:83-115).
 * Every entry point below replaces a piece of that body and cites it.
 *
 * Plain C: pointers, sizes, POD structs.  No torch / PCL / ROS types.
 * A context is NOT thread-safe: one context per (host thread, device).
 * All outputs are owned by the context and stay valid until the next
 * fx_process_batch / fx_destroy on that context.
 */
#ifndef FX_H_
#define FX_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FX_VERSION_MAJOR 0
#define FX_VERSION_MINOR 7

/* pcl::ShapeContext1980: 12 azimuth x 11 elevation x 15 radius bins + rf[9]
 * (ref: include/feature_extraction/feature_extraction_node.h:35-53,75). */
#define FX_DESC_BINS 1980
#define FX_DESC_RF 9
#define FX_DESC_FLOATS 1989 /* 7956 B per keypoint == sizeof(pcl::ShapeContext1980) */
/* pcl::PointDescriptor wire record of ~features (ref: node.h:35-42): x@0 y@4 z@8
 * pad@12 intensity@16 descriptor@20 rf@7940, sizeof 7984 (EIGEN_ALIGN16). */
#define FX_FEATURE_RECORD_BYTES 7984

typedef enum fx_status {
  FX_OK = 0,
  FX_ERR_INVALID_ARG = 1,
  FX_ERR_NO_DEVICE = 2, /* no HIP device / extension unusable: never a CPU fallback */
  FX_ERR_HIP = 3,
  FX_ERR_OOM = 4,
  FX_ERR_TOO_LARGE = 5 /* batch or scan exceeds the limits given to fx_create */
} fx_status;

/* Per-scan flag bits (fx_batch_view.flags).  Capacity overflow never truncates
 * silently: the scan's outputs are then incomplete and the bit says which stage. */
#define FX_FLAG_RING_OVERFLOW 0x1u      /* a ring held more points than limits.max_ring_points */
#define FX_FLAG_CAND_OVERFLOW 0x2u      /* more per-ring candidates than limits.max_candidates */
#define FX_FLAG_KP_OVERFLOW 0x4u        /* more keypoints than limits.max_keypoints */
#define FX_FLAG_NBR_OVERFLOW 0x8u       /* the dense descriptor tier's pools are exhausted (limits.max_dense_points; the scan's
                                         * overflow region holds max_points entries): the keypoint's descriptor is NaN.
                                         * WHICH rows of a batch an exhausted pool fails depends on the order they drew
                                         * their entries in and may differ from run to run; rows that fit never do */
#define FX_FLAG_TOTAL_KP_OVERFLOW 0x10u /* batch-wide keypoint pool exhausted: the pool holds fewer of the scan's descriptor rows
                                         * than it has keypoints (see "Cuts" below) */
#define FX_FLAG_KPC_OVERFLOW 0x20u      /* keypoint_cloud exceeded its pool: the scan's n_kpc is 0 */

/* Cuts (tests/test_gpu_keypoint_cuts.py asserts every clause).
 * - Per scan, max_keypoints: n_keypoints = min(clusters, max_keypoints); the scan keeps its FIRST max_keypoints keypoints in
 *   the reference's order, with the reference's descriptors for them (the 3DSC random ordinals count earlier keypoints only),
 *   and candidates merged into a dropped keypoint report -1.  FX_FLAG_KP_OVERFLOW iff one was dropped.
 * - Per scan, max_kpc_points: a keypoint_cloud that does not fit is not delivered (n_kpc = 0, FX_FLAG_KPC_OVERFLOW); keypoints
 *   and descriptors are unaffected.
 * - Per batch, max_total_keypoints (the descriptor pool of M rows): n_keypoints and kp_offset are NOT clamped to the pool
 *   (kp_offset[B] may exceed M), and keypoints, ~cloud, ~keypoint_cloud and the membership arrays are complete for every
 *   scan — they do not live in the pool.  Descriptor rows exist for pool rows [0, M) only: scan b holds rows
 *   [min(kp_offset[b], M), min(kp_offset[b] + n_keypoints[b], M)), the descriptors of its LEADING keypoints, equal to an uncut
 *   run's.  total_keypoints = min(kp_offset[B], M).  FX_FLAG_TOTAL_KP_OVERFLOW is set exactly on the scans that hold fewer
 *   rows than they have keypoints (a scan without keypoints lost nothing and is not flagged, wherever it lies).
 * - Every egress reports the held rows: FX_OUT_HOST copies total_keypoints rows, the CSR block has total_keypoints rows,
 *   fx_pack_features writes min(total_keypoints, capacity) records; fx_pack_keypoint_records and fx_pack_keypoint_block cut
 *   keypoints at their own capacity (see there), whatever the pool held. */
#define FX_FLAG_INTERNAL 0x40u          /* a self-check of the library failed for this scan (the sliced streaming pass's two
                                           counts of a slice's survivors disagree): its results are not to be trusted — a bug */

/* The 14 ROS private parameters of the reference node (ref: node.cpp:9-34,
 * members node.h:115-127) + the constants the reference hard-codes for the
 * VLP-16 (ref: node.cpp:195, 200, 227), exposed so 64/128-ring sensors work.
 * Doubles/ints exactly as the reference stores them; narrowing to float happens
 * inside, where PCL does it (see oracle/fx_oracle.cpp). */
typedef struct fx_params {
  int32_t cloud_leveling;            /* ref: node.cpp:9   default 1 (host shell concern) */
  double x_min, x_max;               /* ref: node.cpp:14-15  0, 75   */
  double y_min, y_max;               /* ref: node.cpp:16-17  -30, 30 */
  double z_min, z_max;               /* ref: node.cpp:18-19  -1.5, 5 */
  double cluster_tolerance;          /* ref: node.cpp:24  0.65 */
  int32_t cluster_min_count;         /* ref: node.cpp:25  5    */
  int32_t cluster_max_count;         /* ref: node.cpp:26  50   */
  double cluster_radius_threshold;   /* ref: node.cpp:27  0.15 */
  int32_t number_detection_channels; /* ref: node.cpp:28  1    */
  int32_t estimate_descriptors;      /* ref: node.cpp:33  1    */
  double descriptor_radius;          /* ref: node.cpp:34  2.5  */
  /* -- hard-coded in the reference, parameters here -- */
  int32_t n_rings;       /* ref: node.cpp:195  `i<16`                       */
  double el0_deg;        /* ref: node.cpp:200  (i-7)*2-1 at i=0  => -15     */
  double el_step_deg;    /* ref: node.cpp:200  2 deg; window = centre +- step/2 (ref: :201) */
  int32_t secondary_max; /* ref: node.cpp:227  setMaxClusterSize(16)        */
} fx_params;

/* Capacities fixed at fx_create (no allocation in the steady state). 0 = default. */
typedef struct fx_limits {
  uint32_t max_batch;           /* scans per fx_process_batch                       */
  uint32_t max_points;          /* points per scan                                  */
  uint32_t max_ring_points;     /* points per (scan, ring)               (def 2048; <= 32768.  Rings of up to ~2400 points are
                                 * clustered in LDS — azimuth-ordered rings of few runs at any size —, larger ones on scratch
                                 * in HBM: slower, same result) */
  uint32_t max_ring_candidates; /* candidates one ring may emit          (def 256)  */
  uint32_t max_candidates;      /* per-ring candidates per scan, all rings (def 2048; <= 32768.  <= ~3800 live in LDS as points,
                                 * beyond that — up to ~16000 — the large merge tier keeps the coordinates in HBM, beyond
                                 * that everything: slower, same result) */
  uint32_t max_keypoints;       /* keypoints per scan                    (def 256)  */
  uint32_t max_neighbors;       /* support-list slots per keypoint row (def 1024, 4096 for scans of more than 65536
                                 * points; 16 B each, capped at 4096).  Not a cap on the support set: larger sets overflow
                                 * into a per-scan region and take the dense tier */
  uint32_t max_total_keypoints; /* keypoints per batch (descriptor pool) (def max_batch*64) */
  uint32_t max_kpc_points;      /* keypoint_cloud points per scan        (def 4096) */
  uint32_t max_dense_points;    /* support points per batch the dense descriptor tier sorts (rows of more than 1024
                                 * support points; def max(max_batch, 32)*max_points; 28 B each + 17.5 KB per 1024).  New in 0.4 */
  uint32_t max_overflow_points; /* support-list entries beyond max_neighbors a scan's rows may have together (its overflow
                                 * region: 20 B each, per scan of the batch; def max_points, 32/max_batch times that in
                                 * contexts of fewer than 32 scans).  New in 0.6 */
} fx_limits;

/* One scan = what cloudCallback receives after fromPCLPointCloud2
 * (ref: node.cpp:77-81): N points with x,y,z as float at byte offsets 0,4,8 of
 * each record.  stride_bytes = 16 for packed float4 (x,y,z,intensity), 32 for
 * PCL's in-memory pcl::PointXYZI.  Incoming intensity is ignored: the
 * reference overwrites it with the elevation angle (ref: node.cpp:154).
 * roll/pitch are the node's members (ref: node.h:116, set at node.cpp:57-70). */
typedef struct fx_scan_desc {
  const void *points; /* host or device pointer (see FX_IN_DEVICE), 16-byte aligned */
  uint32_t n_points;
  uint32_t stride_bytes; /* multiple of 16 in [16, 256] */
  double roll, pitch;    /* radians; narrowed to float like Eigen::AngleAxisf (ref: node.cpp:163-164) */
} fx_scan_desc;

#define FX_IN_DEVICE 0x1u   /* fx_scan_desc.points are device pointers */
#define FX_OUT_HOST 0x2u    /* copy results to the context's pinned host mirrors and synchronise */
#define FX_OUT_DEBUG 0x4u   /* with FX_OUT_HOST: also copy candidates / membership arrays */
#define FX_OUT_CLOUDS 0x8u  /* with FX_OUT_HOST: also copy the filtered cloud and keypoint_cloud */

/* View of one batch's results.  `d_` = device pointers (always set),
 * `h_` = pinned-host mirrors (set when FX_OUT_HOST, else NULL).
 * Keypoint k of scan b:  keypoints[b*max_keypoints + k]  (x, y, z, elevation_deg)
 *                         = the `~keypoints` cloud (ref: node.cpp:129-131, 238-257).
 * Its descriptor:        descriptors[(kp_offset[b] + k) * FX_DESC_FLOATS ...]
 *                         = pcl::ShapeContext1980 {descriptor[1980], rf[9]} (ref: node.cpp:353).
 * filtered[b*max_points + i], i < n_filtered[b] = the `~cloud` topic (ref: node.cpp:137-139).
 * kpc[b*max_kpc_points + i], i < n_kpc[b] = the `~keypoint_cloud` topic (ref: node.cpp:133-135, 206, 323). */
typedef struct fx_batch_view {
  uint32_t batch;
  uint32_t max_points, max_keypoints, max_candidates, max_kpc_points;
  uint32_t total_keypoints; /* valid only after FX_OUT_HOST */
  /* device */
  const uint32_t *d_n_keypoints; /* [B] */
  const uint32_t *d_kp_offset;   /* [B+1] exclusive prefix of n_keypoints */
  const float *d_keypoints;      /* [B][max_keypoints][4] */
  const float *d_descriptors;    /* [max_total_keypoints][1989]; rows [0, total_keypoints) are this batch's.  READ-ONLY: a row
                                  * keeps its content until a later batch uses it and is then cleared by un-writing what was
                                  * written to it — writing into this buffer corrupts later batches */
  const uint32_t *d_flags;       /* [B] FX_FLAG_* */
  const uint32_t *d_n_filtered;  /* [B] */
  const float *d_filtered;       /* [B][max_points][4] */
  const uint32_t *d_n_kpc;       /* [B] */
  const float *d_kpc;            /* [B][max_kpc_points][4] */
  /* host mirrors */
  const uint32_t *h_n_keypoints;
  const uint32_t *h_kp_offset;
  const float *h_keypoints;
  const float *h_descriptors;
  const uint32_t *h_flags;
  const uint32_t *h_n_filtered;
  const float *h_filtered;
  const uint32_t *h_n_kpc;
  const float *h_kpc;
  /* debug / membership (host mirrors only with FX_OUT_DEBUG) */
  const uint32_t *h_n_candidates;  /* [B]  size of keypoints_full (ref: node.cpp:205) */
  const float *h_candidates;       /* [B][max_candidates][4]  per-ring centroids, ring order */
  const uint32_t *h_cand_size;     /* [B][max_candidates]  points in the per-ring cluster */
  const int32_t *h_cand_keypoint;  /* [B][max_candidates]  keypoint ordinal the candidate merged into, -1 if none */
  const uint32_t *h_kpc_cand;      /* [B][max_kpc_points]  candidate ordinal of each keypoint_cloud point */
  const uint32_t *h_kp_size;       /* [B][max_keypoints]   candidates merged into the keypoint */
  const uint32_t *h_kp_neighbors;  /* [B][max_keypoints]   3DSC neighbours within descriptor_radius */
} fx_batch_view;

/* Per-stage device time of the last batch (HIP events on the context's stream). */
#define FX_N_STAGES 9
typedef struct fx_timings {
  /* k_prep, k_bucket, k_rings_runs (one wavefront per ring), k_rings_large (the second run tier of many-ring sensors + the workgroup ring tier), k_merge (merge tiers
   * small / big / large, k_offsets), k_gather (+ k_rng_ord on small batches; classifies the rows), k_desc_group (k_desc: the
   * group, wave and list rows and the dense stand-in in ONE launch, timed in this slot), k_desc_mid (brackets nothing since
   * that launch took its rows: 0), k_desc_rare (the dense tier's own kernels) */
  float ms[FX_N_STAGES];
  float total_ms;
  /* k_prep's execution span on the device's constant-rate clock: first workgroup's start to last workgroup's end — what
   * rocprofv3 reports as the kernel's duration.  The HIP-event span ms[0] also counts the launch's wait for free CUs,
   * which matters when several contexts keep the GPU busy.  0 when the batch is too old for its clock slot. */
  float k_prep_exec_ms;
} fx_timings;

typedef struct fx_ctx fx_ctx;

uint32_t fx_version(void);
/* ABI guard.  The structs of this header may grow at their END between minor versions (fx_limits did in 0.4 and 0.6) and the
 * library reads every member: a caller compiled against another header must not get as far as fx_create.  Pass the version and
 * the sizes the caller was compiled with (FX_CHECK_ABI() does); FX_ERR_INVALID_ARG, with the mismatch in fx_last_error(),
 * when they are not the library's.  Always initialise fx_params / fx_limits with fx_params_default / fx_params_launch /
 * fx_limits_default of the same library before overriding members. */
fx_status fx_check_abi(uint32_t header_version, size_t sizeof_params, size_t sizeof_limits, size_t sizeof_scan_desc,
                       size_t sizeof_batch_view);
#define FX_CHECK_ABI() \
  fx_check_abi(((uint32_t)FX_VERSION_MAJOR << 16) | FX_VERSION_MINOR, sizeof(fx_params), sizeof(fx_limits), sizeof(fx_scan_desc), sizeof(fx_batch_view))
const char *fx_status_str(fx_status s);
/* message of the last failing call on this thread (HIP error string etc.) */
const char *fx_last_error(void);

/* ref: node.cpp:9-34 (defaults) */
void fx_params_default(fx_params *p);
/* ref: launch/keypoint_playback.launch:17-33 (the preset the launch file sets) */
void fx_params_launch(fx_params *p);
void fx_limits_default(fx_limits *l, uint32_t max_batch, uint32_t max_points);
/* The same for sensors whose keypoints rarely have more than max_neighbors (1024) support points — VLP-16-class scans at the
 * reference's descriptor radius: the dense descriptor tier's pools and the overflow regions hold a few such rows per batch
 * instead of every point of it (1024 scans of 28 800 points: 4.5 GB of device memory instead of 7).  Results are the same;
 * a batch with more dense rows than the pools hold flags them (FX_FLAG_NBR_OVERFLOW), as with any limit.  New in 0.6 */
void fx_limits_sparse(fx_limits *l, uint32_t max_batch, uint32_t max_points);

/* Replaces the FeatureExtractionNode constructor's parameter block (ref: node.cpp:3-34).
 * Allocates every device/host buffer; fails with FX_ERR_NO_DEVICE when no GPU. */
fx_status fx_create(const fx_params *params, const fx_limits *limits, int device_id, fx_ctx **out);
void fx_destroy(fx_ctx *ctx);
/* hipStream_t to launch on (NULL = the context's own stream). */
fx_status fx_set_stream(fx_ctx *ctx, void *hip_stream);
/* The hipStream_t the context launches on (its own unless fx_set_stream gave it another): for event waits and for wrapping
 * it in the caller's framework (torch.cuda.ExternalStream). */
fx_status fx_get_stream(fx_ctx *ctx, void **hip_stream);
/* Streaming mode: batches of up to max_batch scans are replayed as one HIP graph per
 * batch size instead of ~30 separate launches (0 = never).  Needs a non-NULL stream; ignored while
 * profiling is on.  Results are identical either way. */
fx_status fx_set_graph_batch(fx_ctx *ctx, uint32_t max_batch);
/* How many contexts the caller keeps busy on this device at a time (default 1; bench.py and fx::MultiGpu run four).  A
 * launch-policy hint only — results never depend on it: with several batches in flight the grid-stride kernels take
 * smaller grids, so that the batches share the chip instead of each claiming all of it (k_desc's group workgroups: one a CU
 * instead of ten is +2 % on four batches in flight and -10 % on a batch alone).  New in 0.6 */
fx_status fx_set_batches_in_flight(fx_ctx *ctx, uint32_t n);
/* depth > 0: record HIP events around every stage kernel for the next batches, keeping the
 * last `depth` batches; 0 disables.  fx_get_timings reads the batch `back` calls ago
 * (0 = most recent) and waits for it to finish. */
fx_status fx_set_profiling(fx_ctx *ctx, int depth);
/* Restrict the events to some stages (bit i = stage i of fx_timings; default all): every event costs a
 * few microseconds of stream time, so a throughput measurement times only the kernel it needs.  The
 * first and last event of a batch are always recorded (total_ms); untimed stages read 0. */
fx_status fx_set_profiling_stages(fx_ctx *ctx, uint32_t stage_mask);
fx_status fx_get_timings(fx_ctx *ctx, uint32_t back, fx_timings *t);
/* Algorithmic bytes every stage of the LAST batch had to move — what it must read of its inputs plus what it must
 * write of its outputs, each once, from the batch's own counts (points, survivors, ring members, candidates, support
 * points, keypoints); no padding, no re-reads.  The figure a per-kernel roofline fraction divides by the kernel's
 * duration.  Waits for the batch.  (SURVEY.md 8d's per-scan B_alg is the whole path's: bytes[0]'s read + the keypoint
 * and descriptor writes.) */
typedef struct fx_stage_bytes {
  double read[FX_N_STAGES], written[FX_N_STAGES];
} fx_stage_bytes;
fx_status fx_get_stage_bytes(fx_ctx *ctx, fx_stage_bytes *out);
fx_status fx_get_limits(const fx_ctx *ctx, fx_limits *l);

/* Replaces cloudCallback's body for a batch of B scans (ref: node.cpp:83-115):
 * getElevationAngles (:147-156) -> rotateCloud (:159-167) -> filterCloud (:169-183)
 * -> estimateKeypoints (:185-259, getCylinderSegments :261-327)
 * -> estimateDescriptors (:329-355).  Empty scans give K = 0 (ref: :209-210, :263-264). */
fx_status fx_process_batch(fx_ctx *ctx, const fx_scan_desc *scans, uint32_t batch, uint32_t flags,
                           fx_batch_view *out);
/* Wait for the context's stream. */
fx_status fx_synchronize(fx_ctx *ctx);

/* pcl::concatenateFields(keypoints, descriptors) (ref: node.cpp:119): packs the last
 * batch's keypoints + descriptors into 7984-byte pcl::PointDescriptor records on
 * the device.  dst_device must hold total_keypoints records. */
fx_status fx_pack_features(fx_ctx *ctx, void *dst_device, uint32_t capacity_records);

/* ---- PointCloud2 wire formats ----
 * Ingress: what pcl_conversions::toPCL + pcl::fromPCLPointCloud2 do for the node (ref: node.cpp:79-81):
 * pick the float32 fields x, y, z (and optionally intensity) by their byte offsets out of
 * point_step-byte records (extra fields such as `ring` are skipped; point_step may be any size) into
 * the packed float4 layout fx_scan_desc takes.  data_device and dst_device_xyzi are device pointers;
 * dst holds n_points * 16 bytes.  The offsets come from the message's PointField list. */
typedef struct fx_pc2_layout {
  uint32_t point_step;
  uint32_t offset_x, offset_y, offset_z;
  uint32_t offset_intensity; /* 0xffffffff: no such field (the path ignores incoming intensity anyway) */
  uint32_t is_bigendian;
} fx_pc2_layout;
fx_status fx_unpack_pointcloud2(fx_ctx *ctx, const void *data_device, uint32_t n_points, const fx_pc2_layout *layout,
                                void *dst_device_xyzi);
/* Egress: one scan's cloud of the last batch as pcl_ros serialises a PointCloud<PointXYZI>
 * (ref: node.cpp:129-139): 32-byte records, x@0 y@4 z@8 intensity@16 (fields x, y, z, intensity;
 * point_step 32).  dst_device holds capacity_points * 32 bytes; *n_points_out = points written. */
#define FX_CLOUD_KEYPOINTS 0u      /* ~keypoints      */
#define FX_CLOUD_FILTERED 1u       /* ~cloud          */
#define FX_CLOUD_KEYPOINT_CLOUD 2u /* ~keypoint_cloud */
fx_status fx_pack_pointxyzi(fx_ctx *ctx, uint32_t which, uint32_t scan, void *dst_device, uint32_t capacity_points,
                            uint32_t *n_points_out);

/* Fixed-stride keypoint records of the last batch for the cross-GPU gather (one RCCL
 * collective per batch): per scan (1 + rec_keypoints) float4 = {n_kp, flags, 0, 0 as u32}
 * followed by rec_keypoints (x, y, z, elevation) entries, zero padded.  dst_device must hold
 * batch * (1 + rec_keypoints) * 16 bytes. */
fx_status fx_pack_keypoint_records(fx_ctx *ctx, void *dst_device, uint32_t rec_keypoints);

/* The same keypoints as ONE compact block for the cross-GPU gather (0.7): a batch's keypoints packed
 * in scan order behind their offsets, instead of max-stride records (54 keypoints a VLP-16 scan
 * against a stride of 256: a quarter of the bytes on xGMI and in every receiver's HBM).  The block is
 * fx_keypoint_block_bytes(max_scans, max_total_keypoints) bytes whatever the batch holds — every rank
 * hands the collective the same count — as rows of 16 bytes:
 *   row 0                       {scans, keypoints stored, OR of all flags, max_total_keypoints} (u32)
 *   then ceil((max_scans+1)/4)  kp_offset[max_scans + 1] (u32): scan b's keypoints are rows
 *                               [kp_offset[b], kp_offset[b+1]) of the keypoint area; entries beyond
 *                               the batch repeat the total
 *   then ceil(max_scans/4)      flags[max_scans] (u32; 0 beyond the batch)
 *   then max_total_keypoints    (x, y, z, elevation) rows, zero beyond the total
 * A batch with more keypoints than max_total_keypoints is cut there; the scans that lose keypoints
 * (and row 0) carry FX_FLAG_KP_OVERFLOW.  Replaces what the reference would publish per scan on
 * ~keypoints (ref: node.cpp:133-135) for the scans of a whole batch.  Enqueued on the context's
 * stream behind the last fx_process_batch. */
size_t fx_keypoint_block_bytes(uint32_t max_scans, uint32_t max_total_keypoints);
fx_status fx_pack_keypoint_block(fx_ctx *ctx, void *dst_device, uint32_t max_scans, uint32_t max_total_keypoints);

/* ---- Descriptors as compressed rows (CSR) ----
 * A descriptor row has some tens of non-zero words out of 1989.  The CSR block is one fixed-size, self-describing block of
 * fx_descriptor_csr_bytes(max_rows, capacity) bytes, sections 16-byte aligned, in order:
 *   header   {rows, nnz_stored, nnz_needed, rows_stored} (u32)
 *   row_ptr  u32 [max_rows + 1]: row r's entries are [row_ptr[r], row_ptr[r+1]); entries past rows_stored repeat nnz_stored
 *   col      u32 [capacity]: word index 0..1988 of the dense row (bins 0..1979, then rf 1980..1988), increasing within a row
 *   val      f32 [capacity]: that word, bit for bit
 * Rows are the batch's descriptor rows [0, total_keypoints) in d_descriptors order (scan b: [kp_offset[b], kp_offset[b+1])).
 * A word is stored iff its 32-bit pattern is non-zero (-0.0 and NaN are kept; an FX_FLAG_NBR_OVERFLOW row stores every bin):
 * expanding the block into zeros gives the dense rows back bit for bit.  Whole rows are stored in order while they fit
 * `capacity`; the first row that does not fit and every row after it stay empty (rows_stored < rows; nnz_needed is what all
 * rows need).  Nothing is written past capacity.  col / val are separate arrays: (row_ptr, col, val) wrap as a CSR matrix
 * with int32 indices as they are.  New in 0.7 (added symbols only). */
size_t fx_descriptor_csr_bytes(uint32_t max_rows, uint32_t capacity);
/* Packs the last batch's descriptor rows into a CSR block at dst_device (16-byte aligned, fx_descriptor_csr_bytes bytes),
 * enqueued on the context's stream behind the last fx_process_batch.  An empty batch or estimate_descriptors = 0 gives
 * rows = 0; rows > max_rows stores the first max_rows rows (rows_stored <= max_rows).  FX_ERR_TOO_LARGE when the context's
 * descriptor pool could need more than 2^32 - 1 entries (max_total_keypoints > 2 159 383). */
fx_status fx_pack_descriptors_csr(fx_ctx *ctx, void *dst_device, uint32_t max_rows, uint32_t capacity);
/* With FX_OUT_HOST: the host gets the context's own CSR block instead of the dense rows.  h_descriptors is then NULL (the
 * dense host mirror is not allocated for such calls); d_descriptors is unchanged.  Only row_ptr[0..rows], col[0..nnz) and
 * val[0..nnz) cross the link.  Lossless: a batch that needs more entries than the context block holds grows the block
 * (device and pinned mirror) and packs again.  Read the result with fx_get_descriptors_csr. */
#define FX_OUT_DESC_CSR 0x10u
typedef struct fx_descriptor_csr_view {
  uint32_t rows, nnz;
  const uint32_t *h_row_ptr, *h_col; /* pinned host: row_ptr[rows + 1], col[nnz] */
  const float *h_val;                /* pinned host: val[nnz] */
  const uint32_t *d_row_ptr, *d_col; /* the context's device block */
  const float *d_val;
} fx_descriptor_csr_view;
/* The last FX_OUT_HOST | FX_OUT_DESC_CSR batch's rows; valid until the next fx_process_batch (FX_ERR_INVALID_ARG when the
 * last batch was not one). */
fx_status fx_get_descriptors_csr(fx_ctx *ctx, fx_descriptor_csr_view *out);
/* Initial capacity (entries) of the context's CSR block; 0 = the default, max_total_keypoints * 128 (1 KB a row: 8x less
 * than the dense pool; the VLP-16 / 64- / 128-ring test scenes average 15 to 77 non-zero words a row).  Takes effect at the next
 * FX_OUT_DESC_CSR batch; the block still grows when a batch needs more. */
fx_status fx_set_descriptor_csr_capacity(fx_ctx *ctx, uint32_t entries);

/* ---- Matching descriptor rows between scans across azimuth shifts ----
 * PCL's 3DSC draws a random azimuth reference per keypoint (fx_sc3d_xaxis): two descriptors of the same pole differ by an
 * unknown rotation of the 12 azimuth sectors.  A bin index is l*165 + k*15 + j with l the sector, so a rotation by s sectors
 * is a cyclic shift of the column index by 165 s, and rows are matched by trying all 12 (Frome et al., ECCV 2004):
 *   d2(q, t, s) = sum over c < 1980 of (q[c] - t[(c + 165 s) mod 1980])^2        (the 9 rf words are ignored)
 * Both operands are CSR blocks exactly as fx_pack_descriptors_csr writes them ((max_rows, capacity) give the layout, the
 * header gives rows_stored); q_block == t_block matches scans inside one batch.  pairs_host[p] matches the query rows
 * [q_row0, q_row0 + q_rows) against the train rows [t_row0, t_row0 + t_rows); ranges are clipped to each block's
 * rows_stored, a pair with an empty side is legal, and the QUERY ranges of the pairs must be disjoint (FX_ERR_INVALID_ARG
 * otherwise, checked on the host).  Per query row, (train_row, shift, dist2) minimise d2 over the pair's train rows and the
 * enabled shifts — ties to the lowest train row, then the lowest shift —, and (second_row, dist2_second) are the same minimum
 * over the pair's train rows other than train_row.  Every one of the q_max_rows records is written: a row in no pair or
 * clipped away gets train_row = -1, pair = 0xffffffff, dist2 = dist2_second = +inf, flags = 0.  A row that stores any
 * non-finite word — NaN (an FX_FLAG_NBR_OVERFLOW row), +Inf or -Inf, in a bin or in an rf word — never matches and is never
 * matched: train_row = -1 as a query, skipped as a train row.  A row without stored words is an ordinary all-zero
 * descriptor; -0.0 words count as 0.
 * Numerics: dist2 is within 2^-23 d2 + 2^-40 (|q|^2 + |t|^2) + 2^-150 of the exact value (fp64 sums of the exact fp32
 * products, one rounding to fp32 that keeps subnormal results: 2^-150 is half the smallest of them), never negative and
 * never -0.0, exactly +0 for identical rows at shift 0, and the same bits from run to run and with any number of contexts
 * in flight.  Finite rows can be too far apart for fp32: a value of 2^128 - 2^103 or more (FLT_MAX plus half an ulp) is
 * reported as +inf, which orders and ties like any other value, passes max_dist2 = +inf only, and passes max_ratio when
 * dist2_second is +inf too (max_ratio^2 * inf = inf) unless max_ratio is 0 (0 * inf is NaN: rejected).
 * Enqueued on the context's stream; needs no batch to have been processed.  pairs_host is copied before the call returns
 * into a context-owned buffer that grows when a call needs more; nothing else is allocated in the steady state.  New in 0.7
 * (added symbols only). */
typedef struct fx_match_pair { uint32_t q_row0, q_rows, t_row0, t_rows; } fx_match_pair; /* row ranges in the two blocks */
typedef struct fx_match_options {
  uint32_t azimuth_shifts; /* 12 (default) or 1 (shift 0 only) */
  float max_dist2;         /* accept only d2 <= this; +inf = off (default) */
  float max_ratio;         /* accept only d2 <= max_ratio^2 * d2_second (fp32); >= 1 = off (default 1) */
  uint32_t mutual;         /* 1: also compute FX_MATCH_MUTUAL; default 0 */
} fx_match_options;
#define FX_MATCH_ACCEPTED 0x1u /* a best match exists and passes max_dist2 and max_ratio */
#define FX_MATCH_MUTUAL 0x2u   /* (options.mutual) the query row is, for its train_row, the minimiser of (dist2, query row) over
                                * the pair's query rows and all shifts */
typedef struct fx_match { /* 32 B, one per query row */
  int32_t train_row;      /* row in the train block, -1: none */
  uint32_t shift;         /* 0..11 */
  float dist2;
  int32_t second_row;     /* best OTHER train row of the pair, -1: none */
  float dist2_second;     /* +inf when none */
  uint32_t flags;         /* FX_MATCH_* */
  uint32_t pair;          /* index into pairs, 0xffffffff when the row is in no pair */
  uint32_t reserved;      /* 0 */
} fx_match;
void fx_match_options_default(fx_match_options *o);
fx_status fx_match_descriptors_csr(fx_ctx *ctx, const void *q_block_device, uint32_t q_max_rows, uint32_t q_capacity,
                                   const void *t_block_device, uint32_t t_max_rows, uint32_t t_capacity,
                                   const fx_match_pair *pairs_host, uint32_t n_pairs, const fx_match_options *opt,
                                   fx_match *out_device /* [q_max_rows] */);

/* ---- Scan-to-scan rigid motion from the matches ----
 * How the sensor moved between two scans, from their keypoints and the fx_match records that pair them up: a consensus over
 * the matched keypoints and a closed-form least-squares fit, for all pairs of a batch in one launch set.
 * Model (4 degrees of freedom): scans are levelled before anything else (rotateCloud) and the landmarks are near-vertical poles
 * on roughly one plane, so roll and pitch between two scans are neither large nor observable from such points, and a pole
 * centroid's z depends on which rings hit it.  The motion is a rotation about z plus a translation, (c, s, tx, ty) with
 * c^2 + s^2 = 1 fitted on xy only, and tz the mean z difference over the inliers: a query keypoint q maps to
 * (c qx - s qy + tx, s qx + c qy + ty, qz + tz), which should be its train keypoint.  Full SE(3) is out of scope.
 * Inputs: the two keypoint blocks are exactly what fx_pack_keypoint_block writes ((max_scans, max_total_keypoints) give the
 * layout); row r of the keypoint area is descriptor row r of the same batch, and row 0's "keypoints stored" bounds the valid
 * rows.  matches_device and pairs_host are what the caller gave to and got from fx_match_descriptors_csr; pair index p here
 * is the `pair` field there.  The QUERY ranges of the pairs must be disjoint (FX_ERR_INVALID_ARG otherwise, as are hyp_corr
 * outside 2..128, min_inliers < 2 and an inlier_dist or min_baseline that is not finite and positive; nothing is launched).
 * Outputs: every one of the n_pairs records is written and, when inlier_device is given, every one of its q_max_rows words
 * (1 = the row is in the final inlier set of its pair, else 0); nothing beyond them.
 * Correspondences of pair p: in ascending query row, the rows i of [q_row0, q_row0 + q_rows) clipped to q_max_rows with
 * m[i].pair == p, m[i].train_row >= 0, (m[i].flags & require_flags) == require_flags, i below the query block's and
 * m[i].train_row below the train block's keypoints stored, and all six coordinates (x, y, z of both keypoints) finite.  Only
 * the first FX_REG_MAX_CORR are used (FX_REG_TRUNCATED when there are more); n_corr is the number used.
 * Sample pool: the H = min(n_corr, hyp_corr) correspondences of lowest (dist2 bits as uint32, query row); samples are the
 * pairs (a, b), a < b, of pool ranks in lexicographic order.
 * Hypothesis stage — fp32 in exactly this operation order, no contraction, no fma, correctly rounded divide and sqrt; with
 * (qx, qy) -> (tx, ty) the keypoints of a correspondence and differences taken as b - a:
 *   lq2 = dqx dqx + dqy dqy, lt2 = dtx dtx + dty dty; skip unless lq2 >= mb mb and lt2 >= mb mb (mb = min_baseline);
 *   skip if |sqrt(lq2) - sqrt(lt2)| > 2 inlier_dist;
 *   dot = dqx dtx + dqy dty, crs = dqx dty - dqy dtx, nrm = sqrt(dot dot + crs crs); skip unless nrm > 0;
 *   c = dot / nrm, s = crs / nrm; midpoints mq = (qa + qb) 0.5, mt likewise;
 *   tx = mtx - (c mqx - s mqy), ty = mty - (s mqx + c mqy);
 *   correspondence i agrees iff rx rx + ry ry <= inlier_dist inlier_dist, rx = ((c qx - s qy) + tx) - t_x,
 *   ry = ((s qx + c qy) + ty) - t_y.
 * The winner is the sample with the most agreeing correspondences among all n_corr, ties to the lowest (a, b); a sample with
 * fewer than 2 agreeing is no hypothesis.  numpy float32 reproduces this stage bit for bit; counts and the winner are integers.
 * Scale: multiplying every coordinate, inlier_dist and min_baseline by 2^k multiplies every intermediate of the stage by a power
 * of two, so the integers and the bits of c and s stay and tx, ty scale exactly — but only while no intermediate leaves fp32's
 * normal range.  The widest is the operand of nrm's root: dot dot + crs crs = |dq|^2 |dt|^2 in exact arithmetic, the fourth
 * power of the sample's baseline b = sqrt(|dq| |dt|).  It is normal for 2^-126 <= b^4 < 2^128, that is 2^-31.5 m <= b < 2^32 m
 * (6.7e-10 m .. 4.3e9 m).  Outside:
 *   2^-37.25 m <= b < 2^-31.5 m   the sum is subnormal and has lost bits: the sample stands, c and s no longer scale exactly;
 *   b < 2^-37.25 m (b^4 < 2^-149) the sum rounds to 0, nrm = 0 and the sample is skipped by nrm > 0, distinct keypoints or not;
 *   b >= 2^32 m                   the sum is +inf and so is nrm: c = s = 0 while dot and crs are finite (the transform sends every
 *                                 keypoint to the sample's train midpoint, which is half a train baseline from its own two
 *                                 keypoints: it gathers no agreement from them), NaN once dot or crs overflow as well (b >= 2^64 m);
 *                                 a NaN agrees with nothing.  Where lq2 or lt2 is +inf the length gate compares a NaN
 *                                 (inf - inf) and lets the sample through: it ends here all the same.
 * A pair all of whose samples lie outside the band is FX_REG_NO_HYPOTHESIS.  min_baseline is squared in fp32: below 2^-75
 * (2.6e-23) the square rounds to 0 and the baseline gate passes everything, coincident keypoints included; nrm > 0 is then the
 * one clause that keeps 0 / 0 out.  The default min_baseline of 2 m keeps every sample that passes the gate 32 binades inside
 * the band.  tests/test_gpu_register_numerics.py runs all of this against numpy.
 * Refit — fp64, sequential in ascending query row, no contraction, over the winner's agreeing set:
 *   centroids qc, tc of the set (sum, then divide); per member with u = q - qc, v = t - tc:
 *   Sdot += (ux vx + uy vy), Scrs += (ux vy - uy vx); nrm = sqrt(Sdot Sdot + Scrs Scrs);
 *   c = Sdot / nrm, s = Scrs / nrm when nrm > 0, else the (c, s) the fit started from (the hypothesis's, widened to double);
 *   tx = tcx - (c qcx - s qcy), ty = tcy - (s qcx + c qcy).
 * All n_corr correspondences are then tested again under this transform in fp64 (same residual expression; the threshold is
 * the double product of the float inlier_dist with itself), which gives the set I1; if I1 has at least 2 members the fit is
 * run once more over I1, otherwise the first fit and its set stay.  The reported inliers are the set the final transform was
 * fitted to; tz is the sequential mean of t_z - q_z over it (fp64), rms = sqrt(sum r^2 / n) under the final transform, the
 * fp64 value rounded once.  FX_REG_VALID iff n_inliers >= min_inliers.  A pair with FX_REG_NO_HYPOTHESIS carries the
 * identity (c = 1, s = 0), tx = ty = tz = 0, rms = +inf, n_inliers = 0, hyp_a = hyp_b = 0xffffffff.
 * The same bits from run to run and with any number of contexts in flight: every decision is an integer or an ordered,
 * correctly rounded operation, and no sum runs in completion order.
 * Enqueued on the context's stream; needs no batch to have been processed.  pairs_host is copied before the call returns
 * into a context-owned buffer that grows when a call needs more; nothing else is allocated in the steady state.  New in 0.7
 * (added symbols only). */
#define FX_REG_MAX_CORR 1024u
typedef struct fx_register_options {
  float inlier_dist;      /* xy distance (m) within which a correspondence agrees with a transform; default 0.30 */
  float min_baseline;     /* a 2-correspondence hypothesis needs both point pairs at least this far apart (m); default 2.0 */
  uint32_t hyp_corr;      /* hypotheses are formed from the hyp_corr best correspondences; 2..128, default 64 */
  uint32_t min_inliers;   /* FX_REG_VALID needs at least this many final inliers; >= 2, default 3 */
  uint32_t require_flags; /* FX_MATCH_* bits a match record must carry to be used; default FX_MATCH_ACCEPTED */
} fx_register_options;
#define FX_REG_VALID 0x1u         /* a transform was fitted to >= min_inliers correspondences */
#define FX_REG_TRUNCATED 0x2u     /* more than FX_REG_MAX_CORR (1024) correspondences: the first 1024 in query-row order were used */
#define FX_REG_NO_HYPOTHESIS 0x4u /* fewer than 2 correspondences, or no sample passed the gates */
typedef struct fx_registration { /* 64 B, one per pair */
  double c, s, tx, ty, tz;
  float rms;                     /* xy residual over the final inliers, the fp64 value rounded once */
  uint32_t n_corr, n_inliers, flags;
  uint32_t hyp_a, hyp_b;         /* query rows of the winning sample, 0xffffffff when none */
} fx_registration;
void fx_register_options_default(fx_register_options *o);
fx_status fx_register_matches(fx_ctx *ctx,
    const void *q_kp_block_device, uint32_t q_max_scans, uint32_t q_max_total_keypoints,
    const void *t_kp_block_device, uint32_t t_max_scans, uint32_t t_max_total_keypoints,
    const fx_match *matches_device, uint32_t q_max_rows,
    const fx_match_pair *pairs_host, uint32_t n_pairs, const fx_register_options *opt,
    fx_registration *out_device /* [n_pairs] */, uint32_t *inlier_device /* [q_max_rows] or NULL */);

/* ---- Chaining the motions into a trajectory and the inliers into landmark tracks ----
 * The last step of pack -> match -> register for ONE batch of consecutive scans of one sensor: the match and the register were
 * run with q_block == t_block and the pairs "scan p + 1 (query) onto scan p (train)", p = 0 .. scans - 2 (what
 * capi.pairs_consecutive builds), so reg[p] maps scan p + 1's frame into scan p's.  The poses of all scans in one common frame,
 * the rows that are the same physical pole followed from scan to scan, and each pole's mean position in that frame come out of
 * one launch set, from exactly the buffers the three calls left on the device.  Out of scope: "B sensors, this batch against
 * the last" (two blocks), continuing tracks across calls, and any re-estimation of the motions (no bundle adjustment);
 * init_pose_host lets a caller continue the POSES across calls when two batches overlap by one scan.
 * Sizes: S = min(n_scans, the block's scans, max_scans) scans and rows = min(the block's keypoints stored,
 * max_total_keypoints, q_max_rows) rows take part.  scan(r) is the b < S with kp_offset[b] <= r < kp_offset[b + 1]; a row at or
 * beyond kp_offset[S] or `rows` belongs to nothing (a non-row).
 * Good links: link p (p < S - 1) is good iff reg[p].flags & FX_REG_VALID and c, s, tx, ty, tz of reg[p] are all finite.
 * Poses — an fp64 left fold in scan order, no contraction, no fma, no renormalisation of (c, s); p* is the pose before, r* the
 * link's record:
 *   P_0 = init_pose (the identity c = 1, s = tx = ty = tz = 0 when NULL), segment 0, flags 0 (init_pose's own segment and flags
 *   are ignored);
 *   good link b - 1: c = pc rc - ps rs, s = ps rc + pc rs, tx = (pc rtx - ps rty) + ptx, ty = (ps rtx + pc rty) + pty,
 *   tz = ptz + rtz; segment kept, flags 0;
 *   bad link b - 1: the pose of scan b - 1 as it is, segment + 1, FX_POSE_GAP;
 *   b >= S: the pose and segment of the scan before, flags = FX_POSE_NO_SCAN only.
 * All n_scans poses are written.  numpy float64 reproduces the fold bit for bit.
 * Kept links: row r of scan b >= 1 proposes the parent t = matches[r].train_row iff inlier[r] == 1, matches[r].pair == b - 1,
 * link b - 1 is good, kp_offset[b - 1] <= t < kp_offset[b], t < rows, and x, y, z of both rows are finite (the fourth word, the
 * elevation, is not a coordinate).  These conditions also make any garbage record memory-safe.  A parent keeps its proposer of
 * LOWEST row (an integer minimum: order-free); every other proposer starts a track of its own and counts in n_conflicts.
 * A track is a maximal chain of kept links; every row is in exactly one.  Links join consecutive scans only and never cross a
 * bad link, so a track's observation at depth d lies in scan first_scan + d and a track has at most one row a scan.
 * Landmarks: the tracks of at least min_obs observations, numbered by ascending first row (the row of lowest scan).
 * landmark_of_row[r] is that number, -1 for rows of shorter tracks and for non-rows; all q_max_rows words are written.
 * obs_row holds the landmarks' rows grouped by landmark in landmark order, ascending scan inside each; entries from n_obs on are
 * 0xffffffff; all q_max_rows words are written.
 * Fusing — fp64, sequential in obs_row order, no contraction; (x, y, z) the row's float coordinates widened, (c, s, tx, ty, tz)
 * its scan's pose: wx = (c x - s y) + tx, wy = (s x + c y) + ty, wz = z + tz.  The landmark's x, y, z are the sums of wx, wy, wz
 * from 0.0 in that order, each divided once by (double)n_obs.  rms_xy: a second pass in the same order, acc += (dx dx + dy dy)
 * with dx = wx - x, dy = wy - y; rms_xy = (float)sqrt(acc / (double)n_obs), the fp64 value rounded once.
 * Capacity: the landmarks [0, min(n_landmarks, max_landmarks)) are written and nothing behind them; header.n_landmarks is the
 * number needed; landmark_of_row and obs_row are complete either way.
 * header: scans = S, rows, n_landmarks, n_obs (the landmarks' observations), n_conflicts, n_gaps (bad links below S), 0, 0.
 * FX_ERR_INVALID_ARG with the reason in fx_last_error(), nothing launched: a NULL required pointer (landmarks_device may be
 * NULL with max_landmarks == 0, reg_device with n_scans == 1, the row arrays with q_max_rows == 0; opt NULL = the defaults),
 * n_scans == 0 or n_scans > max_scans, min_obs == 0, an init_pose whose c, s, tx, ty or tz is not finite, a keypoint block not
 * 16-byte or records not 8-byte (words: 4-byte) aligned.
 * The same bytes from run to run and with any number of contexts in flight: every decision is an integer (32-bit integer
 * atomics only, minimum and sum), every fp64 value an ordered chain of correctly rounded operations on one lane.
 * Enqueued on the context's stream; needs no batch to have been processed.  init_pose_host is copied before the call returns.
 * Scratch is a context-owned buffer that grows when a call has more rows; nothing is allocated in the steady state.  New in 0.7
 * (added symbols only). */
typedef struct fx_pose {            /* 48 B: scan b's frame -> the frame of init_pose (scan 0's when NULL) */
  double c, s, tx, ty, tz;
  uint32_t segment, flags;
} fx_pose;
#define FX_POSE_GAP 0x1u            /* the link into this scan was unusable: pose held from the scan before, segment + 1 */
#define FX_POSE_NO_SCAN 0x2u        /* b is beyond the block's scans: pose held, nothing else */
typedef struct fx_landmark {        /* 48 B */
  double x, y, z;                   /* mean of the observations in the common frame */
  float rms_xy;                     /* sqrt(mean xy distance^2 of the observations from (x, y)); fp64, rounded once */
  uint32_t n_obs, obs0;             /* its observations are obs_row[obs0 .. obs0 + n_obs), ascending scan */
  uint32_t first_row, first_scan, last_scan;
} fx_landmark;
typedef struct fx_track_header {    /* 32 B */
  uint32_t scans, rows, n_landmarks, n_obs, n_conflicts, n_gaps, reserved[2];
} fx_track_header;
typedef struct fx_track_options {
  uint32_t min_obs;                 /* a track becomes a landmark with at least this many observations; >= 1, default 2 */
  uint32_t reserved;
} fx_track_options;
void fx_track_options_default(fx_track_options *o);
fx_status fx_track_landmarks(fx_ctx *ctx,
    const void *kp_block_device, uint32_t max_scans, uint32_t max_total_keypoints,   /* fx_pack_keypoint_block */
    const fx_match *matches_device, const uint32_t *inlier_device, uint32_t q_max_rows,
    const fx_registration *reg_device, uint32_t n_scans,        /* reg[p], p < n_scans - 1: scan p + 1 -> scan p */
    const fx_pose *init_pose_host /* NULL: identity */, const fx_track_options *opt,
    fx_pose *poses_device /* [n_scans] */, int32_t *landmark_of_row_device /* [q_max_rows] */,
    uint32_t *obs_row_device /* [q_max_rows] */, fx_landmark *landmarks_device, uint32_t max_landmarks,
    fx_track_header *header_device);

/* ---- Carrying the landmark tracks across batches: a persistent map on the device ----
 * fx_track_landmarks numbers the landmarks of ONE batch from 0.  A sensor run is many batches; the map gives every landmark one id
 * for the whole run and one running mean.  The caller cuts the run into batches that OVERLAP BY ONE SCAN (batch k + 1 starts with
 * the scan batch k ended with), runs process -> pack -> match -> register -> track on each with init_pose_host = the map's
 * last_pose, and hands the track's buffers to fx_map_update.  A scan's keypoints never depend on the batch it is in, so the overlap
 * scan's rows are the same bits in the same order in both batches, and a track of batch k + 1 that begins at local row j of its
 * scan 0 is the continuation of the track of batch k that ended at local row j of its last scan: an integer decision.  The pose
 * fold continues bit for bit through init_pose and a landmark's mean is a sequential fp64 sum divided once, so a map that
 * continues the sums holds what ONE batch of the whole run would have produced, bit for bit, however the run is cut (for tracks
 * run with min_obs == 2; see the limits below).
 * The map is owned by the context it was created on (destroy it before the context) and updated by a launch set on that context's
 * stream: no host synchronisation, no allocation in the steady state.  Its accumulators (the running sums, the anchor, the carry
 * table and a copy of the carry scan's rows) are private; fx_map_landmark and fx_map_header are what a caller reads.
 * Inputs of fx_map_update: exactly what the fx_track_landmarks call before it was given (the keypoint block and its layout,
 * q_max_rows, max_landmarks) and what it wrote (poses, landmark_of_row, obs_row, landmarks, header); every count is read from the
 * track's header on the device.  Anything else is memory-safe and unspecified.
 * Sizes: S and rows are the track header's scans and rows (clipped to max_scans and to min(max_total_keypoints, q_max_rows): the
 * same numbers when the arguments are the track's); L = min(the header's n_landmarks, max_landmarks); when n_landmarks exceeds
 * max_landmarks FX_MAP_TRACK_TRUNCATED is set and the first L are used (rows of the others report -1).  The rows of scan b are
 * [min(kp_offset[b], rows), min(kp_offset[b + 1], rows)).  A batch of S == 0 counts in `batches`, sets last_joined = last_new = 0
 * and changes nothing else.
 * Overlap: with FX_MAP_OVERLAP the caller states that this batch's scan 0 is the previous batch's last scan.  It is ACCEPTED iff
 * the map has seen a scan (scans > 0), carry_rows equals the row count of scan 0, and all four words of every row of scan 0 equal
 * the stored copy of the carry scan's rows, compared as 32-bit patterns.  Flag given and not accepted: FX_MAP_OVERLAP_MISMATCH
 * is set and the batch is taken as without the flag.
 * Numbering: scan_base = scans - 1 when accepted, else scans; seg_base = segments - 1 (the previous batch's last global segment)
 * when accepted, else segments (0 for the first batch).  Afterwards scans = scan_base + S and segments = seg_base +
 * poses[S - 1].segment + 1.
 * Joins: batch landmark i < L CONTINUES map landmark g iff the overlap is accepted, its first_scan == 0 and
 * g = carry[first_row - kp_offset[0]] >= 0.  Every other one is NEW and gets the ids n_needed, n_needed + 1, ... in the batch's
 * landmark order: ids are order of appearance.  An id at or beyond the map's max_landmarks counts in n_needed and is not stored:
 * FX_MAP_FULL is set, its rows report -1 and carry -1, and its continuation in a later batch is new again.
 * Accumulation — fp64, one lane a landmark, sequential in obs_row order, no contraction, no fma.  wx, wy, wz of an observation are
 * fx_track_landmarks's fusing clause word for word: (c x - s y) + tx, (s x + c y) + ty, z + tz from the row's float coordinates and
 * its scan's pose in poses_device.  A new landmark starts Sx = Sy = Sz = Dx = Dy = Q = 0.0, takes the first observation's
 * (wx, wy) as its anchor (ax, ay) and adds every observation; a continued one keeps its sums and its anchor, SKIPS its first
 * observation (the overlap row, counted in the batch before) and adds the rest.  Adding an observation: Sx += wx, Sy += wy,
 * Sz += wz, dx = wx - ax, dy = wy - ay, Dx += dx, Dy += dy, Q += (dx dx + dy dy).
 * Records, with n = (double)n_obs of the landmark so far: x = Sx / n, y = Sy / n, z = Sz / n; mx = Dx / n, my = Dy / n,
 * var = Q / n - (mx mx + my my), taken as 0 unless var > 0; rms_xy = (float)sqrt(var) (the spread about the mean through the
 * anchor: not the track's two-pass value, equal to it within rounding).  last_scan = scan_base + the batch landmark's last_scan;
 * a new landmark's first_scan = scan_base + its local first_scan, segment = seg_base + poses[local first_scan].segment, flags 0;
 * a continued one gains FX_MAP_LM_CONTINUED.
 * map_id_of_row[r]: the map id of row r's batch landmark; -1 for rows of no landmark, non-rows and landmarks not stored.  All
 * q_max_rows words are written when the pointer is given.
 * Carry for the next call, for every local row j of scan S - 1: the map id of the batch landmark that holds the row; otherwise
 * the old carry[j] when S == 1 and the overlap was accepted (a batch of only the overlap scan changes nothing); otherwise -1.
 * The rows of scan S - 1 are copied as the new carry scan.  A last scan of more rows than max_carry_rows stores no carry:
 * carry_rows = 0 and the next overlap is a mismatch.
 * header: n_landmarks = min(n_needed, max_landmarks) records stored; n_obs the observations accumulated into stored landmarks;
 * last_joined / last_new this update's continued / new landmarks (new: stored or not); last_pose = poses[S - 1] as the track
 * wrote it: what the caller passes as the next init_pose_host.
 * FX_ERR_INVALID_ARG with the reason in fx_last_error(), nothing launched, the map unchanged: a NULL required pointer
 * (landmarks_device may be NULL with max_landmarks == 0, the row arrays with q_max_rows == 0, map_id_of_row_device always), a map
 * of another context, max_landmarks == 0 at create, unknown flag bits, a keypoint block not 16-byte or records not 8-byte (words:
 * 4-byte) aligned.
 * The same bytes from run to run and with any number of contexts in flight: every decision is an integer (32-bit integer atomics
 * only, or and sum), every fp64 value an ordered chain of correctly rounded operations on one lane.
 * Limits: tracks are continued only across an accepted one-scan overlap; a pole seen again after a missed detection, a bad link or
 * after leaving the field of view enters as a new landmark.  fx_map_merge (below) folds such fragments back into one landmark
 * within a segment and fx_map_join_segments (below) brings two segments a bad link left into one frame; after long drift fragments
 * stay apart until fx_map_close_loop (below) closes the loop: fx_map_relocalize finds the pose of a
 * scan in the map without a prior and fx_map_localize refines it, which gives the closure its prior.  The equality with one batch of the whole run
 * holds for min_obs == 2; with a larger min_obs a track that a batch edge cuts into pieces that are each too short is missed.
 * n_obs and n_needed are 32-bit counts.  FX_MAP_FULL is sticky and n_needed only rises under fx_map_update; fx_map_compact (below)
 * gives the room of absorbed and let-go landmarks back, fx_map_export_host / fx_map_import_host carry a map to another context,
 * and fx_map_append / fx_map_append_host (below) put a second map behind this one instead of replacing it.
 * fx_map_create allocates all of the map's buffers and enqueues its first reset; fx_map_reset enqueues the state of a fresh map;
 * fx_map_update's scratch is a context-owned buffer that grows when a call has a larger max_landmarks.  fx_map_get returns the
 * device addresses of the header and the records (stable for the map's life; read them in stream order); fx_map_read_header and
 * fx_map_read_landmarks copy to the host and wait for the stream (records [first, first + count) within max_landmarks).  New in
 * 0.7 (added symbols only). */
#define FX_MAP_OVERLAP 0x1u           /* fx_map_update flags: scan 0 of this batch is the last scan of the batch before */
#define FX_MAP_FULL 0x1u              /* header flags, sticky: a landmark was not stored (n_needed > max_landmarks) */
#define FX_MAP_OVERLAP_MISMATCH 0x2u  /* ... an update's FX_MAP_OVERLAP was not accepted */
#define FX_MAP_TRACK_TRUNCATED 0x4u   /* ... a track header's n_landmarks exceeded the max_landmarks of its records */
#define FX_MAP_LM_CONTINUED 0x1u      /* fx_map_landmark flags: continued across at least one batch edge */
typedef struct fx_map fx_map;
typedef struct fx_map_landmark {      /* 48 B */
  double x, y, z;                     /* mean of the observations so far, in the frame of the run's first init_pose */
  float rms_xy;
  uint32_t n_obs, first_scan, last_scan, segment, flags; /* scans and segment: global numbers of the run */
} fx_map_landmark;
typedef struct fx_map_header {        /* 88 B */
  uint32_t n_landmarks, n_needed, n_obs, scans, batches, segments, flags, carry_rows, last_joined, last_new;
  fx_pose last_pose;
} fx_map_header;
fx_status fx_map_create(fx_ctx *ctx, uint32_t max_landmarks, uint32_t max_carry_rows, fx_map **out);
void fx_map_destroy(fx_map *map);
fx_status fx_map_reset(fx_ctx *ctx, fx_map *map);
fx_status fx_map_update(fx_ctx *ctx, fx_map *map,
    const void *kp_block_device, uint32_t max_scans, uint32_t max_total_keypoints,           /* what the track was given */
    const fx_pose *poses_device, const int32_t *landmark_of_row_device, const uint32_t *obs_row_device, uint32_t q_max_rows,
    const fx_landmark *landmarks_device, uint32_t max_landmarks, const fx_track_header *track_header_device, /* what it wrote */
    uint32_t flags /* FX_MAP_OVERLAP */, int32_t *map_id_of_row_device /* [q_max_rows] or NULL */);
fx_status fx_map_get(fx_map *map, const fx_map_header **header_device, const fx_map_landmark **landmarks_device);
fx_status fx_map_read_header(fx_ctx *ctx, fx_map *map, fx_map_header *out_host);
fx_status fx_map_read_landmarks(fx_ctx *ctx, fx_map *map, uint32_t first, uint32_t count, fx_map_landmark *out_host);

/* ---- Merging the fragments of one pole in the map: spatial re-association ----
 * A track is a chain of links between CONSECUTIVE scans: one missed detection, one match that is no inlier or one conflict breaks
 * it, and the pole enters the map again under a new id with a second mean.  Inside one segment the poses are one consistent frame,
 * so the fragments of one pole lie centimetres apart there while two poles never do; fx_map_merge joins fragments that are close
 * in xy and disjoint in time.  It is enqueued on the context's stream (no host synchronisation, no allocation in the steady state:
 * its scratch is a context-owned buffer sized by the map's max_landmarks), may be called after any fx_map_update, any number of
 * times, and changes nothing of a map it is never called on.
 * The alias table is private memory of the map, int32 [max_landmarks]: alias[id] == -1, the landmark is live; otherwise the id of
 * the live landmark that absorbed it — always fully resolved, never a chain.  fx_map_create and fx_map_reset fill it with -1,
 * fx_map_update never touches it.
 * ONE CALL, with N = header.n_landmarks and the records and sums as they are when it starts:
 * Live set: landmark i < N takes part iff alias[i] == -1, n_obs >= 1 and its record's x and y are finite.
 * Eligibility: g may precede h iff both take part, g != h, segment[g] == segment[h], last_scan[g] < first_scan[h],
 * first_scan[h] - last_scan[g] <= max_gap_scans and d2 <= md md, where dx = x[g] - x[h], dy = y[g] - y[h], d2 = dx dx + dy dy in
 * fp64 (no contraction, no fma) and md = (double)merge_dist.  Two landmarks ever seen in the same scan are never merged: that keeps
 * two close but distinct poles apart.
 * Proposal: every h with such a g proposes the one of greatest last_scan (the most recent: the track resumes where it stopped);
 * ties go to the smallest d2, compared as the uint64 bit patterns of the non-negative doubles, then to the lowest id.
 * Acceptance: a g keeps, among its proposers, the one of lowest first_scan, ties to the lowest id (one 64-bit integer atomic
 * minimum on (first_scan << 32) | h: order-free).  last_scan strictly grows along a kept link and a landmark has at most one kept
 * link in and one out, so the kept links form simple chains.
 * Fold: a chain's root r is its member without a kept predecessor; one lane folds the members m1, m2, ... into r in chain order,
 * fp64, no contraction.  For each m, with nm = (double)n_obs[m] and ex = ax[m] - ax[r], ey = ay[m] - ay[r] (the anchors):
 * Sx[r] += Sx[m] (Sy, Sz likewise); Q[r] += ((Q[m] + 2.0 (ex Dx[m] + ey Dy[m])) + nm (ex ex + ey ey)); Dx[r] += (Dx[m] + nm ex),
 * Dy[r] += (Dy[m] + nm ey); n_obs[r] += n_obs[m]; last_scan[r] = last_scan[m]; flags[r] |= FX_MAP_LM_MERGED and m's
 * FX_MAP_LM_CONTINUED; m gains FX_MAP_LM_ABSORBED and alias[m] = r, and everything else of its record stays as it was (frozen).
 * Then r's x, y, z and rms_xy are recomputed from its sums by fx_map_update's "Records" clause; its first_scan, segment and
 * anchor are unchanged.
 * Re-pointing: every alias entry that pointed at a landmark absorbed by this call is set to that landmark's root, and every
 * carry entry >= 0 is replaced by its root, so the next fx_map_update continues the merged landmark.  The header is untouched:
 * ids are stable and never compacted by this call, n_obs only moved (fx_map_compact, below, is the call that renumbers).
 * Result (when given): proposals = the h that proposed, merged = the kept links, live = the landmarks that take part after the
 * call, reserved = 0.
 * One call is one round: a fragment whose proposal was not kept (another fragment resumed the same track earlier) is picked up by
 * the next call; call until merged == 0 for a fixpoint, on which a further call changes no byte.
 * The same bytes from run to run and with any number of contexts in flight: every decision is an integer or a minimum over a
 * total order, every fp64 value an ordered chain on one lane.  The search structure (a hashed grid) never shows in the result.
 * FX_ERR_INVALID_ARG with the reason in fx_last_error(), nothing launched, the map unchanged: a NULL ctx or map (fx_map_get_alias:
 * a NULL out pointer), a map of another context, merge_dist not finite and positive, max_gap_scans == 0, result_device not 4-byte
 * aligned; fx_map_read_alias: entries outside max_landmarks.
 * Limits: merging happens within one segment only (fx_map_join_segments, below, makes one segment of two; twins that drift
 * holds beyond merge_dist are fx_map_close_loop's, below, to bring together first;
 * fx_map_relocalize and fx_map_localize, below, give the
 * transform between a scan's frame and the map's, without and with a prior pose; they join nothing).  Chained merges of one call may join A and C that are up to
 * 2 merge_dist apart, through B.  The map_id_of_row arrays of earlier batches keep the absorbed ids: resolve them through the
 * alias table (id = alias[id] >= 0 ? alias[id] : id); the absorbed records, their sums and their alias entries stay until
 * fx_map_compact (below) takes them out.  A cell of the grid that holds very many fragments is searched by one lane
 * a landmark: time, not the result, grows with the square of a cell's population.
 * fx_map_get_alias returns the table's device address (stable for the map's life; read it in stream order); fx_map_read_alias
 * copies entries [first, first + count) to the host and waits for the stream.  New in 0.7 (added symbols only). */
#define FX_MAP_LM_ABSORBED 0x2u  /* fx_map_landmark flags: merged into another landmark (see the alias table); the record is frozen */
#define FX_MAP_LM_MERGED   0x4u  /* this landmark has absorbed at least one other */
typedef struct fx_map_merge_options {
  float merge_dist;        /* xy gate in metres between the two means; finite and > 0; default 0.30 (fx_register_options.inlier_dist's default) */
  uint32_t max_gap_scans;  /* a fragment may resume at most this many scans after its predecessor ended; >= 1; default 64 */
} fx_map_merge_options;
typedef struct fx_map_merge_result { uint32_t proposals, merged, live, reserved; } fx_map_merge_result; /* 16 B */
void fx_map_merge_options_default(fx_map_merge_options *o);
fx_status fx_map_merge(fx_ctx *ctx, fx_map *map, const fx_map_merge_options *opt /* NULL: defaults */,
                       fx_map_merge_result *result_device /* or NULL */);
fx_status fx_map_get_alias(fx_map *map, const int32_t **alias_device);            /* [max_landmarks], stable for the map's life */
fx_status fx_map_read_alias(fx_ctx *ctx, fx_map *map, uint32_t first, uint32_t count, int32_t *out_host);

/* ---- Localising scans against the map: relocalisation with a prior pose ----
 * Everything above places a scan in the map's frame by dead reckoning: the track folds pairwise motions and the map continues that
 * fold.  fx_map_localize compares scans with the map itself: given the scans of a keypoint block, a PRIOR pose for each and a
 * map, it finds which landmark each keypoint is and fits each scan's pose in the map's frame.  It is what joining the segments a
 * bad link leaves, bounding drift and "map once, localise later" all start from.  It is enqueued on the context's stream (no
 * host synchronisation, no allocation in the steady state: its scratch is a context-owned buffer sized by the map's
 * max_landmarks and by q_max_rows, shared with fx_map_merge) and READS the map only: header, records, sums, alias and carry are bit
 * for bit what they were.  Call it after a track (prior_poses_device = the track's poses_device) or alone against a finished map.
 * Sizes: S = min(n_scans, the block's scans, max_scans) and rows = min(the block's keypoints stored, max_total_keypoints,
 * q_max_rows), scan(r) and the non-rows exactly as in fx_track_landmarks.  All n_scans records and all q_max_rows words of both
 * row arrays are written and nothing beyond them.  A scan b >= S gets FX_LOC_NO_SCAN and nothing else: the prior as its pose, D =
 * the identity (dc = 1, ds = dtx = dty = dtz = 0), rms = +inf, n_corr = n_inliers = 0, hyp_a = hyp_b = 0xffffffff.  A scan b < S
 * whose prior's c, s, tx, ty or tz is not finite gets FX_LOC_BAD_PRIOR and the same record.  Non-rows and the rows of such scans
 * get -1 in both row arrays.
 * Eligible landmarks: with N = header.n_landmarks as it is when the call runs, g < N is eligible iff alias[g] == -1, n_obs >=
 * min_landmark_obs, its x, y and z are finite and its segment passes opt.segment: FX_LOC_ANY_SEGMENT passes every segment,
 * FX_LOC_LAST_SEGMENT stands for header.segments - 1 read on the device (nothing is eligible in a map of no segment), any other
 * value is the global segment number itself.
 * Association, per row r of scan b whose x, y and z are finite: (wx, wy, wz) is the row under the prior, fx_track_landmarks's
 * fusing clause word for word (the same device function).  dx = x[g] - wx, dy = y[g] - wy, d2 = dx dx + dy dy in fp64, no
 * contraction; g is in reach iff d2 <= sd sd, sd = (double)search_dist.  nearest_of_row[r] is the eligible g in reach of lowest
 * (d2 as uint64 bits, id), -1 when there is none or the row is not finite.  Several rows may pick the same landmark.
 * Correspondences of scan b: its rows with nearest >= 0, in ascending row; the first FX_LOC_MAX_CORR are used (FX_LOC_TRUNCATED
 * when there are more); n_corr is the number used.  Correspondence i carries q = (wx, wy, wz) and t = (x, y, z) of its landmark,
 * all double.
 * Hypothesis stage: fx_register_matches's clause word for word with every operation in fp64 (map coordinates are not small): the
 * pool is the H = min(n_corr, hyp_corr) correspondences of lowest (d2 bits, row); the samples (a, b), a < b, in lexicographic
 * order; the gates, c, s, the midpoints, tx, ty and the agreement test are the same expressions in the same order, with mb mb
 * and inlier_dist inlier_dist the double products of the floats widened and 2 inlier_dist the double product 2.0 (double)
 * inlier_dist.  The winner has the most agreeing correspondences among all n_corr, ties to the lowest (a, b); a sample with fewer
 * than 2 agreeing is no hypothesis.  Without one the scan gets FX_LOC_NO_HYPOTHESIS, D = the identity, rms = +inf, n_inliers = 0
 * and the prior as its pose.  numpy float64 reproduces the stage bit for bit.
 * Scale: fx_register_matches's statement with fp64's range: dot dot + crs crs is normal for 2^-1022 <= b^4 < 2^1024, that is
 * 2^-255.5 m <= b < 2^256 m; it rounds to 0 (the sample is skipped) below 2^-268.5 m (b^4 < 2^-1074) and is +inf (c = s = 0 or
 * NaN: no agreement) from 2^256 m.  mb mb is the double product of a float: never 0, so the baseline gate cannot be disabled.
 * Refit: fx_register_matches's clause word for word (the same device code): the fit over the agreeing set, the re-test of all
 * n_corr giving I1, the second fit when I1 has at least 2 members.  (dc, ds, dtx, dty) is the final transform, dtz the sequential
 * mean of t_z - q_z over the final set, rms and n_inliers as in the register; hyp_a, hyp_b the rows of the winning sample.
 * Pose: FX_LOC_VALID iff n_inliers >= min_inliers.  The pose is then the track's good-link composition of D with the prior p:
 * c = dc pc - ds ps, s = ds pc + dc ps, tx = (dc ptx - ds pty) + dtx, ty = (ds ptx + dc pty) + dty, tz = ptz + dtz.  Otherwise
 * it is the prior's five doubles, bit for bit; D is reported all the same.  segment and flags of the pose are the prior's.
 * map_id_of_row[r]: the landmark of row r when r is in its scan's final inlier set, else -1.
 * One call is one round: the output poses are fx_pose records, so a second round takes them as its priors (with a smaller
 * search_dist).  A search distance of 2 m bounds the prior's error after one bad link; the association is right only where that
 * error is below half the local pole spacing, and the consensus takes care of the rest.
 * FX_ERR_INVALID_ARG with the reason in fx_last_error(), nothing launched, no output byte touched: a NULL required pointer (the
 * row arrays may be NULL only with q_max_rows == 0, nearest_of_row_device always), a map of another context, n_scans == 0 or
 * n_scans > max_scans, search_dist, inlier_dist or min_baseline not finite and positive, hyp_corr outside 2..128, min_inliers < 2,
 * min_landmark_obs == 0, reserved != 0, a keypoint block not 16-byte or records not 8-byte (words: 4-byte) aligned.
 * The same bytes from run to run and with any number of contexts in flight: every decision is an integer or a minimum over a
 * total order, every fp64 sum an ordered chain on one lane.  The search structure (fx_map_merge's hashed grid, cell edge
 * sd (1 + 2^-8)) never shows in the result.
 * Limits: a prior is needed: fx_map_relocalize (below) produces one from the map's geometry alone (the map stores no descriptors),
 * and this call refines it; the call joins no segments (fx_map_join_segments, below, does, and takes a record's dc as its prior) and
 * re-estimates no landmark (fx_map_observe, below, does, from this call's records and its row-to-landmark table): it produces the
 * poses and the table both start from.  A cell of the grid that
 * holds very many landmarks is walked by one lane a row.  New in 0.7 (added symbols only). */
#define FX_LOC_MAX_CORR 1024u
#define FX_LOC_ANY_SEGMENT  0xffffffffu
#define FX_LOC_LAST_SEGMENT 0xfffffffeu   /* header.segments - 1, read on the device; nothing is eligible in a map of no segment */
typedef struct fx_localize_options {
  float search_dist;      /* xy gate of the association under the prior, m; finite, > 0; default 2.0 */
  float inlier_dist;      /* as fx_register_options; default 0.30 */
  float min_baseline;     /* as fx_register_options; default 2.0 */
  uint32_t hyp_corr;      /* 2..128, default 64 */
  uint32_t min_inliers;   /* >= 2, default 3 */
  uint32_t min_landmark_obs; /* a landmark takes part with at least this many observations; >= 1, default 2 */
  uint32_t segment;       /* only landmarks of this global segment take part; default FX_LOC_LAST_SEGMENT */
  uint32_t reserved;      /* 0 */
} fx_localize_options;
#define FX_LOC_VALID 0x1u         /* a correction was fitted to >= min_inliers correspondences: pose = D o prior */
#define FX_LOC_TRUNCATED 0x2u     /* more than FX_LOC_MAX_CORR correspondences: the first 1024 in row order were used */
#define FX_LOC_NO_HYPOTHESIS 0x4u /* fewer than 2 correspondences, or no sample passed the gates */
#define FX_LOC_BAD_PRIOR 0x8u     /* the prior's c, s, tx, ty or tz is not finite */
#define FX_LOC_NO_SCAN 0x10u      /* b is beyond the block's scans */
typedef struct fx_localization {   /* 112 B, one per scan */
  fx_pose pose;                    /* VALID: D o prior; otherwise the prior, bit for bit.  segment, flags: the prior's */
  double dc, ds, dtx, dty, dtz;    /* D: the correction in the map frame */
  float rms;
  uint32_t n_corr, n_inliers, flags;
  uint32_t hyp_a, hyp_b;           /* rows of the winning sample, 0xffffffff: none */
} fx_localization;
void fx_localize_options_default(fx_localize_options *o);
fx_status fx_map_localize(fx_ctx *ctx, fx_map *map,
    const void *kp_block_device, uint32_t max_scans, uint32_t max_total_keypoints,
    const fx_pose *prior_poses_device, uint32_t n_scans, uint32_t q_max_rows, const fx_localize_options *opt /* NULL: defaults */,
    fx_localization *out_device /* [n_scans] */, int32_t *map_id_of_row_device /* [q_max_rows] */,
    int32_t *nearest_of_row_device /* [q_max_rows] or NULL */);

/* ---- Finding a scan's pose in the map without a prior: global relocalisation from the pole constellation ----
 * fx_map_localize needs a prior within about search_dist of the truth, and only dead reckoning from the run that built the map
 * gives one.  A later run that starts somewhere in a stored map ("map once, localise later") and a segment that a bad link cut off
 * have none.  fx_map_relocalize finds the pose from the scan's keypoints and the map's positions alone: it lays pairs of keypoints
 * (seeds) on pairs of landmarks of the same length and scores each rigid transform that results by the keypoints it lands on a
 * landmark.  The intended use is one fx_map_relocalize, then fx_map_localize with pose as the prior and a small search_dist
 * (2 inlier_dist), which refits the pose over all correspondences.  It is enqueued on the context's stream (no host
 * synchronisation, no allocation in the steady state: its scratch is the context-owned buffer the other map calls share, grown
 * as needed) and READS the map only: header, records, sums, alias, carry and the carry scan are bit for bit what they were.
 * Every floating-point step is fp64, no contraction, no fma; id, pt, mb, xb are inlier_dist, pair_tol, min_baseline and
 * max_baseline widened to double.
 * Sizes, non-rows, scans b >= S: exactly as in fx_map_localize.  All n_scans records and all q_max_rows words are written and
 * nothing beyond them.  A scan b >= S gets flags = FX_RELOC_NO_SCAN, n_kp = n_seeds = 0, n_hyp = 0 and otherwise the record of a
 * scan without a winner (below).
 * Eligible landmarks: fx_map_localize's clause word for word with this call's min_landmark_obs and segment: g < N is eligible iff
 * alias[g] == -1, n_obs >= min_landmark_obs, its x, y and z are finite and its segment passes opt.segment.
 * Used keypoints of scan b: its rows whose x, y and z are finite, in ascending row, at most the first FX_RELOC_MAX_KP (more:
 * FX_RELOC_TRUNCATED); their coordinates are the floats widened to double, in the scan's own frame.  n_kp is the number used;
 * keypoint k is the k-th of them.
 * Seeds: the candidates are the pairs (a, b), a < b, of used keypoints with mb mb <= d2 <= xb xb, dx = x[b] - x[a], dy = y[b] - y[a],
 * d2 = dx dx + dy dy.  They are ranked by descending d2 (compared as uint64 bit patterns), then ascending (a, b); the seeds are the
 * first n_seeds = min(count, max_seeds): long baselines fix the yaw best.
 * Hypotheses: for the seed of rank s with keypoints (a, b), every ordered pair (g, h), g != h, of eligible landmarks: the
 * transform is fx_register_matches's hypothesis clause in fp64 (the device function fx_map_localize uses) of the correspondences
 * A = (x[a], y[a], X[g], Y[g]) and B = (x[b], y[b], X[h], Y[h]), with mb mb as the baseline gate (both lengths) and pt in the place
 * of 2 inlier_dist as the length gate: |sqrt(lq2) - sqrt(lt2)| > pt is gated out.  A pair that is gated out is no hypothesis.
 * n_hyp counts the hypotheses of the scan over all its seeds.
 * Score of a hypothesis (c, s, tx, ty): the number of used keypoints k whose image wx = (c x - s y) + tx, wy = (s x + c y) + ty has
 * an eligible landmark with d2 <= id id, dx = X[g] - wx, dy = Y[g] - wy, d2 = dx dx + dy dy.  Two keypoints on one landmark both
 * count.
 * Winner: the hypothesis of highest score, ties to the lowest (s, g, h).  A scan whose best score is below 2 or that has no
 * hypothesis is WITHOUT A WINNER: flags = FX_RELOC_NO_HYPOTHESIS (and FX_RELOC_TRUNCATED when it applies), the identity pose
 * (c = 1, s = tx = ty = tz = 0, segment 0, flags 0), score = runner_up = 0, seed_a = seed_b = lm_a = lm_b = 0xffffffff; n_kp,
 * n_seeds and n_hyp are what they are.
 * Rivals (the ambiguity test: poles in a row or a lattice admit several poses): with T* the winner's transform and a*, b* its
 * seed keypoints, another hypothesis T is a rival iff for q = a* or q = b* the vector r = T(q) - T*(q), taken componentwise from
 * the two images in the expression above, has r.x r.x + r.y r.y > g g, g = 2.0 id.  runner_up is the highest score among the
 * rivals, 0 when there is none.  The hypotheses that restate the winner's pose from other seeds or landmarks are no rivals.
 * Result: FX_RELOC_VALID iff score >= min_inliers and score - runner_up >= min_margin; FX_RELOC_AMBIGUOUS iff score >=
 * min_inliers and the margin fails; neither below min_inliers.  Whenever there is a winner: pose (c, s, tx, ty) is its transform;
 * the landmark of a keypoint is the eligible landmark of lowest (d2 as uint64 bits, id) among those with d2 <= id id of its image
 * (the SCORED keypoints are those that have one); tz is the sequential sum, in ascending row, of Z[landmark] - z over the scored
 * keypoints, divided by (double)score; pose.segment is the segment of landmark g, pose.flags 0; seed_a, seed_b are the rows of a, b
 * and lm_a, lm_b the landmarks g, h.  map_id_of_row[r] is the landmark of row r for the scored rows of a VALID scan and -1
 * everywhere else.
 * FX_ERR_INVALID_ARG with the reason in fx_last_error(), nothing launched, no output byte touched: a NULL required pointer
 * (map_id_of_row_device may be NULL only with q_max_rows == 0), a map of another context, n_scans == 0 or n_scans > max_scans,
 * inlier_dist, pair_tol or min_baseline not finite and positive, max_baseline not finite or below min_baseline, max_seeds outside
 * 1..64, min_inliers < 3, min_margin == 0, min_landmark_obs == 0, reserved != 0, a keypoint block not 16-byte or records not 8-byte
 * (words: 4-byte) aligned.
 * The same bytes from run to run and with any number of contexts in flight: every decision is an integer (32- and 64-bit integer
 * atomics only, sum and maximum) or a minimum over a total order, every fp64 value an ordered chain on one lane.  The search
 * structures (two of fx_map_merge's hashed grids, one with a cell edge from max_baseline + pair_tol for the landmark pairs and one
 * from inlier_dist for the score) and the reduction never show in a result; numpy float64 reproduces every record bit for bit.
 * Limits: the pose is that of ONE two-point hypothesis, centimetres off under noise: refine it with fx_map_localize.  The work
 * grows with seeds x eligible landmarks x the landmarks whose distance matches the seed x keypoints, and the rivals cost a second
 * pass; max_seeds and max_baseline bound it.  A scan whose poles repeat a pattern of the map (a row, a lattice) comes back
 * AMBIGUOUS; a scan of fewer than three poles the map holds cannot be VALID.  The call joins no segments (fx_map_join_segments,
 * below) and writes nothing to the map.  New in 0.7 (added symbols only). */
#define FX_RELOC_MAX_KP 64u
typedef struct fx_relocalize_options {   /* 40 B */
  float inlier_dist;      /* a keypoint lands on a landmark within this xy distance, m; finite, > 0; default 0.30 */
  float pair_tol;         /* allowed difference between a seed's length and a landmark pair's; finite, > 0; default 0.30 */
  float min_baseline;     /* shortest seed pair, m; finite, > 0; default 2.0 */
  float max_baseline;     /* longest seed pair, m; finite, >= min_baseline; default 60.0 */
  uint32_t max_seeds;     /* seed pairs tried per scan; 1..64, default 16 */
  uint32_t min_inliers;   /* score needed for FX_RELOC_VALID; >= 3, default 4 */
  uint32_t min_margin;    /* lead needed over the best rival; >= 1, default 1 */
  uint32_t min_landmark_obs; /* a landmark takes part with at least this many observations; >= 1, default 2 */
  uint32_t segment;       /* as fx_localize_options.segment; default FX_LOC_ANY_SEGMENT */
  uint32_t reserved;      /* 0 */
} fx_relocalize_options;
#define FX_RELOC_VALID 0x1u         /* score >= min_inliers and score - runner_up >= min_margin */
#define FX_RELOC_TRUNCATED 0x2u     /* more than FX_RELOC_MAX_KP finite rows: the first 64 in row order were used */
#define FX_RELOC_NO_HYPOTHESIS 0x4u /* no hypothesis, or none that lands 2 keypoints */
#define FX_RELOC_AMBIGUOUS 0x8u     /* score >= min_inliers, but a rival pose scores within min_margin of it */
#define FX_RELOC_NO_SCAN 0x10u      /* b is beyond the block's scans */
typedef struct fx_relocalization {   /* 96 B, one per scan */
  fx_pose pose;                      /* the winner's transform scan -> map; the identity without a winner */
  uint64_t n_hyp;                    /* hypotheses of the scan */
  uint32_t n_kp, n_seeds, score, runner_up, flags;
  uint32_t seed_a, seed_b;           /* rows of the winning seed, 0xffffffff: none */
  uint32_t lm_a, lm_b;               /* the landmarks they were laid on, 0xffffffff: none */
  uint32_t reserved;                 /* 0 */
} fx_relocalization;
void fx_relocalize_options_default(fx_relocalize_options *o);
fx_status fx_map_relocalize(fx_ctx *ctx, fx_map *map,
    const void *kp_block_device, uint32_t max_scans, uint32_t max_total_keypoints,
    uint32_t n_scans, uint32_t q_max_rows, const fx_relocalize_options *opt /* NULL: defaults */,
    fx_relocalization *out_device /* [n_scans] */, int32_t *map_id_of_row_device /* [q_max_rows] */);

/* ---- Folding localised scans into the map: the landmarks re-estimated from what fx_map_localize matched ----
 * A landmark's mean otherwise moves only through a track handed to fx_map_update: a localisation run against a finished map ("map
 * once, localise later") leaves every landmark's sums, n_obs, x, y, z and rms_xy as the mapping run left them, however often the
 * poles are seen again.  fx_map_observe folds the inlier rows of localised scans into the landmarks they were matched to.  It takes
 * what the fx_map_localize (or fx_map_relocalize: its records begin with the same fx_pose, but carry other flags) call before it was
 * given and what it wrote, reads both on the device, and is enqueued on the context's stream: no host read stands between the two
 * calls, no host synchronisation, no allocation in the steady state (its scratch is the context-owned buffer of fx_map_merge, sized
 * by the map's max_landmarks and by q_max_rows).  One call covers the whole (row, landmark) table as it is when the call runs on
 * the stream.
 * Sizes: S, rows, scan(r) and the non-rows exactly as in fx_map_localize; N = header.n_landmarks, clipped to the map's
 * max_landmarks.
 * Used scans: scan b < S is used iff (loc[b].flags & require_flags) == require_flags and c, s, tx, ty and tz of loc[b].pose are all
 * finite.  require_flags == 0 uses every scan of a finite pose; a pose that is not finite is never used.  scans_used counts them.
 * Proposals: row r < rows of a used scan proposes iff its x, y and z are finite and id = map_id_of_row[r] satisfies 0 <= id < N.
 * Anything else is not a proposal: -1, garbage, ids at or beyond N, a table from before a compaction.  That makes the call
 * memory-safe on any table.  `proposed` counts the proposals.
 * Target: g = alias[id] >= 0 ? alias[id] : id: a merge since the localise is followed, and two ids of one root are one landmark
 * from here on.  The proposal is STALE, and counted in `stale`, unless g < N, alias[g] == -1, n_obs[g] >= 1 and the record's x, y
 * and z are finite.
 * Gate: (wx, wy, wz) is the row under loc[b].pose, fx_track_landmarks's fusing clause word for word (the same device function).
 * With the record as it is when the call starts: dx = x[g] - wx, dy = y[g] - wy, d2 = dx dx + dy dy in fp64, no contraction; the
 * proposal passes iff d2 <= gd gd, gd = (double)gate_dist; one that fails counts in `gated`.  Observations of an earlier scan of the
 * same call do not move the gate of a later one.
 * One observation a scan a landmark: among the passing proposals of one scan with the same g the one of lowest (d2 as uint64 bits,
 * row) is kept, the others count in `duplicates`; `added` is the number kept.  proposed = added + duplicates + gated + stale.
 * Fold: every landmark g with k >= 1 kept observations takes them in ascending row, which is ascending scan: fx_map_update's
 * "Adding an observation" clause word for word on g's sums with g's anchor, one fp64 chain on one lane.  Then n_obs[g] += k; x, y,
 * z and rms_xy are recomputed by fx_map_update's "Records" clause; flags |= FX_MAP_LM_OBSERVED; first_scan, last_scan, segment and
 * the anchor are untouched.  landmarks_touched counts these landmarks.
 * Header: n_obs += added, and nothing else.  Alias, carry, the carry scan and every untouched record and its sums keep their bytes.
 * Outputs, every word written in both modes: observed_id_of_row[r], all q_max_rows words: g for a kept observation, else -1;
 * gained_of_landmark[i], all max_landmarks words: the k of landmark i, else 0; result: eight words, reserved = 0.
 * FX_OBS_DRY_RUN: the three outputs are what the applying call would have written, and the map is bit for bit what it was.
 * FX_ERR_INVALID_ARG with the reason in fx_last_error(), nothing launched, no output byte touched, the map unchanged: a NULL ctx,
 * map, kp_block_device or loc_device; a NULL map_id_of_row_device with q_max_rows != 0; a map of another context; n_scans == 0 or
 * n_scans > max_scans; gate_dist not finite and positive; unknown require_flags bits; an unknown mode; reserved != 0; a keypoint
 * block not 16-byte, records not 8-byte, word arrays not 4-byte aligned.
 * The same bytes from run to run and with any number of contexts in flight: every decision is an integer or a minimum over a total
 * order (32-bit integer atomics only, sums), every fp64 sum an ordered chain on one lane; no floating-point atomics anywhere.
 * Limits: the call creates no landmark: unmatched rows are ignored.  It does not touch scan numbers: first_scan and last_scan
 * place a landmark in the mapping run's trajectory (the merge's disjointness and the loop closure's weights rest on that), and a
 * localised scan is not part of that trajectory.  Scans that also go through fx_map_update are counted twice, and nothing detects
 * that.  n_obs is a 32-bit count.  One lane folds a landmark's list and every entry of a list is ranked against the whole list:
 * time, not the result, grows with the longest list.  New in 0.7 (added symbols only).
 * The call removes no landmark either: fx_map_expect (below) counts, from the same inputs, how often each landmark should have
 * been seen and how often it was, and fx_map_retire (below fx_map_compact) takes out the ones those counts condemn.
 * The landmarks this call does not create, fx_map_discover (below fx_map_expect) does: from the unmatched rows of the same inputs. */
#define FX_MAP_LM_OBSERVED 0x8u   /* fx_map_landmark flags: gained at least one observation through fx_map_observe */
#define FX_OBS_APPLY 0u
#define FX_OBS_DRY_RUN 1u         /* report everything, change no byte of the map */
typedef struct fx_map_observe_options {   /* 16 B */
  float gate_dist;        /* an observation must lie within this xy distance of its landmark's mean; finite, > 0; default 0.30 */
  uint32_t require_flags; /* FX_LOC_* bits a scan's record must carry to be used; default FX_LOC_VALID */
  uint32_t mode;          /* FX_OBS_APPLY (default), FX_OBS_DRY_RUN */
  uint32_t reserved;      /* 0 */
} fx_map_observe_options;
typedef struct fx_map_observe_result {    /* 32 B */
  uint32_t scans_used, proposed, added, duplicates, gated, stale, landmarks_touched, reserved;
} fx_map_observe_result;
void fx_map_observe_options_default(fx_map_observe_options *o);
fx_status fx_map_observe(fx_ctx *ctx, fx_map *map,
    const void *kp_block_device, uint32_t max_scans, uint32_t max_total_keypoints,   /* what the localise was given */
    const fx_localization *loc_device, uint32_t n_scans,                            /* what it wrote */
    const int32_t *map_id_of_row_device, uint32_t q_max_rows,
    const fx_map_observe_options *opt /* NULL: defaults */, fx_map_observe_result *result_device /* or NULL */,
    uint32_t *gained_of_landmark_device /* [max_landmarks] or NULL */, int32_t *observed_id_of_row_device /* [q_max_rows] or NULL */);

/* ---- Negative evidence: per landmark, how often localised scans should have seen it and how often they did ----
 * A pole that was cut down, a sign that was moved, a false landmark from a parked lorry: fx_map_compact lets go only of short, old
 * landmarks, and a real pole that stood for a thousand scans passes both tests for ever.  fx_map_expect counts, for every landmark,
 * the scans of a localised run that should have seen it (expected) and the scans that did (seen); fx_map_retire (below
 * fx_map_compact) takes out the landmarks that are expected again and again and never seen.  The inputs are exactly
 * fx_map_observe's, so the two calls can follow one fx_map_localize in either order (fx_map_relocalize records under the same
 * caveat as there).  The call is enqueued on the context's stream: no host read, no host synchronisation, no allocation in the
 * steady state (its scratch is the context-owned buffer of fx_map_merge, sized by the map's max_landmarks and by q_max_rows).  It
 * READS the map only: a snapshot before and after is byte-identical.  Every floating-point step is fp64 with no contraction and
 * no fma, and every float (a keypoint's x and y, the options) is widened to double first.
 * Sizes: S, rows, scan(r) and the non-rows exactly as in fx_map_localize; N = header.n_landmarks, clipped to the map's
 * max_landmarks.
 * Used scans: scan b < S is used iff (loc[b].flags & require_flags) == require_flags and c, s, tx, ty and tz of loc[b].pose are all
 * finite.  require_flags == 0 uses every scan of a finite pose; a pose that is not finite is never used.  scans_used counts them.
 * Eligible landmarks: with N = header.n_landmarks as it is when the call runs, g < N is eligible iff alias[g] == -1, n_obs >=
 * min_landmark_obs, its x, y and z are finite and its segment passes opt.segment: FX_LOC_ANY_SEGMENT passes every segment,
 * FX_LOC_LAST_SEGMENT stands for header.segments - 1 read on the device (nothing is eligible in a map of no segment), any other
 * value is the global segment number itself.
 * Naming: row r < rows of a used scan proposes iff its x, y and z are finite and id = map_id_of_row[r] satisfies 0 <= id < N
 * (anything else proposes nothing: -1, garbage, ids at or beyond N; that makes the call memory-safe on any table).  Its target is
 * g = alias[id] >= 0 ? alias[id] : id.  If g is eligible the row NAMES g; otherwise it counts in `stale` and names nothing.
 * Geometry of an eligible g at (X, Y) under the used scan b of pose (c, s, tx, ty): dx = X - tx, dy = Y - ty, d2 = (dx dx) + (dy dy),
 * lx = (c dx) + (s dy), ly = (c dy) - (s dx), l2 = (lx lx) + (ly ly): (lx, ly) is the landmark in the scan's levelled sensor frame.
 * In range iff lo2 <= d2 <= hi2, lo2 = (double)min_range (double)min_range, hi2 = (double)max_range (double)max_range.  d2 is taken
 * in the map frame on purpose: it is the form the grid's one-cell-apart proof covers.  A NaN fails.
 * In box iff x_min <= lx <= x_max and y_min <= ly <= y_max.  Keypoints are centroids of points that survived the pass-through box
 * in the levelled sensor frame, so the box, not a cone, is this sensor's field of view.
 * Seen(b, g) iff in range and some row of scan b names g.
 * Shadowed(b, g) iff shadow_width > 0 and some row k of scan b, at (kx, ky) widened, meets all of: kx, ky and kz are finite (its id
 * does not matter); it does not name g; k2 = (kx kx) + (ky ky) < l2; (kx lx) + (ky ly) > 0; with crs = (kx ly) - (ky lx): (crs crs)
 * <= (w2 l2), w2 = (double)shadow_width (double)shadow_width.  In words: a detected object stands nearer on the same ray (within
 * shadow_width of it), so not seeing g is no evidence.
 * Expected(b, g) iff in range and (Seen or (in box and not Shadowed)).  Hence seen <= expected for every landmark, always.
 * Counts: expected[g] = the number of used scans b with Expected(b, g), seen[g] the number with Seen(b, g).  FX_EXPECT_WRITE: all
 * max_landmarks words of both arrays are written, 0 where nothing counts.  FX_EXPECT_ADD: a word whose count is non-zero gains it in
 * uint32 arithmetic (wrapping); every other word keeps its bytes: the caller zeroes the arrays once and accumulates over many calls.
 * Result (when given), 32 B: scans_used; in_range, in_box, shadowed, expected and seen are counts of pairs (b, g), b used and g
 * eligible: in_range the pairs in range, in_box those in range and in box, shadowed those in range, in box, not seen and shadowed;
 * stale as above; landmarks_expected the number of landmarks with a non-zero expected count from this call.
 * FX_ERR_INVALID_ARG with the reason in fx_last_error(), nothing launched, no output byte touched: a NULL ctx, map,
 * kp_block_device or loc_device; a NULL map_id_of_row_device with q_max_rows != 0; either count array NULL; a map of another
 * context; n_scans == 0 or n_scans > max_scans; x_min > x_max or y_min > y_max or a bound that is NaN; min_range not finite or
 * negative; max_range not finite, not positive or below min_range; shadow_width not finite or negative; unknown require_flags bits;
 * min_landmark_obs == 0; mode > 1; reserved != 0; a keypoint block not 16-byte, records not 8-byte, word arrays not 4-byte aligned.
 * The same bytes from run to run and with any number of contexts in flight: every decision is a comparison of correctly rounded
 * fp64 values, every count a 32-bit integer sum (integer atomics only; no floating-point atomics anywhere), and the search
 * structure (fx_map_merge's hashed grid with the cell edge max_range (1 + 2^-8)) never shows in a byte.
 * Limits: z takes no part: a centroid's z depends on the rings that hit it.  Occlusion by things that are not keypoints (a wall, a
 * lorry) is unknowable here: it is what fx_map_retire's ratio is for.  Scans also folded by fx_map_update are counted like any
 * other.  The counters are the caller's, not the map's: the snapshot format does not change.  One lane takes a landmark in range
 * and walks the scan's rows: time, not the result, grows with rows x landmarks in range.  New in 0.7 (added symbols only). */
#define FX_EXPECT_WRITE 0u
#define FX_EXPECT_ADD 1u          /* add this call's non-zero counts to the arrays, leave every other word alone */
typedef struct fx_map_expect_options {    /* 48 B */
  float x_min, x_max, y_min, y_max;  /* the field of view in the levelled sensor frame; default 1, 74, -29, 29: fx_params_default's box drawn in by 1 m */
  float min_range, max_range;        /* xy distance sensor to landmark; finite, 0 <= min <= max, max > 0; default 2.0, 60.0 */
  float shadow_width;                /* half width of a nearer keypoint's shadow; finite, >= 0, 0: no shadows; default 0.5 */
  uint32_t require_flags;            /* FX_LOC_* bits a scan's record must carry to be used; default FX_LOC_VALID */
  uint32_t min_landmark_obs;         /* >= 1; default 2 */
  uint32_t segment;                  /* FX_LOC_ANY_SEGMENT (default), FX_LOC_LAST_SEGMENT or a segment number */
  uint32_t mode;                     /* FX_EXPECT_WRITE (default), FX_EXPECT_ADD */
  uint32_t reserved;                 /* 0 */
} fx_map_expect_options;
typedef struct fx_map_expect_result {     /* 32 B */
  uint32_t scans_used, in_range, in_box, shadowed, expected, seen, stale, landmarks_expected;
} fx_map_expect_result;
void fx_map_expect_options_default(fx_map_expect_options *o);
/* Host only: the context's pass-through box (fx_params x_min .. y_max) drawn in by `margin` on every side, computed in float
 * ((float)x_min + margin, (float)x_max - margin, ...), and the defaults otherwise. */
void fx_map_expect_options_from_params(const fx_params *params, float margin, fx_map_expect_options *o);
fx_status fx_map_expect(fx_ctx *ctx, fx_map *map,
    const void *kp_block_device, uint32_t max_scans, uint32_t max_total_keypoints,   /* what the localise was given */
    const fx_localization *loc_device, uint32_t n_scans,                            /* what it wrote */
    const int32_t *map_id_of_row_device, uint32_t q_max_rows,
    const fx_map_expect_options *opt /* NULL: defaults */, fx_map_expect_result *result_device /* or NULL */,
    uint32_t *expected_of_landmark_device /* [max_landmarks] */, uint32_t *seen_of_landmark_device /* [max_landmarks] */);

/* ---- Learning new poles: the unexplained rows of localised scans that fall on one spot again and again made landmarks ----
 * fx_map_observe re-estimates the landmarks the scans matched and fx_map_expect / fx_map_retire take out the ones that are gone;
 * a pole put up after the mapping run stays an unmatched row in every scan for ever.  fx_map_discover lets it enter the map: the
 * rows of used scans that name no landmark and stand nowhere near a known one, yet fall within join_dist of one spot of the map
 * frame in at least min_obs scans of the call, become a landmark.  The inputs are exactly fx_map_observe's and fx_map_expect's, so
 * the three calls can follow one fx_map_localize.  The call is enqueued on the context's stream: no host read, no host
 * synchronisation, no allocation in the steady state (its scratch is the context-owned buffer of fx_map_merge, sized by the map's
 * max_landmarks and by q_max_rows).  Every floating-point step is fp64 with no contraction and no fma; kd = (double)known_dist,
 * jd = (double)join_dist; a d2 is dx dx + dy dy; "d2 bits" is its uint64 pattern.
 * Sizes: S, rows, scan(r) and the non-rows exactly as in fx_map_localize; N = header.n_landmarks, clipped to the map's
 * max_landmarks.
 * Segment: seg is opt.segment, FX_LOC_LAST_SEGMENT standing for header.segments - 1 read on the device.  The call is REFUSED when
 * that resolves to nothing (a map of no segment) or seg >= header.segments: refused = 1, every other result word 0 except first_id
 * (below), every word of new_id_of_row -1, and the map keeps every byte.
 * Used scans: scan b < S is used iff (loc[b].flags & require_flags) == require_flags and c, s, tx, ty and tz of loc[b].pose are all
 * finite (fx_map_observe's clause).  scans_used counts them.
 * Unmatched rows: row r < rows of a used scan is unmatched iff its x, y and z are finite, map_id_of_row[r] < 0 and its world point
 * (wx, wy, wz) under loc[b].pose (fx_track_landmarks's fusing clause word for word, the same device function) is finite in all
 * three.  An id >= 0 is never dereferenced: the call is memory-safe on any table.  `unmatched` counts these rows.
 * Known: an unmatched row is known iff some g < N has alias[g] == -1, n_obs[g] >= 1, finite x[g] and y[g], segment[g] == seg and,
 * with dx = x[g] - wx, dy = y[g] - wy, d2 <= kd kd: the merge's live set, and the segment.  There is no min_landmark_obs: young
 * landmarks explain rows too.  `known` counts these rows; the other unmatched rows are FREE (free_rows).
 * Leaders: a free row r is a leader iff no free row r' < r has d2 <= jd jd, dx = wx[r'] - wx[r], dy = wy[r'] - wy[r].  Leaders are
 * pairwise further than jd apart and the predicate is a pure function of the set of free rows.  `leaders` counts them.
 * Attachment: every free row attaches to the leader l of lowest (d2 bits, l) among the leaders with d2 <= jd jd; a leader
 * attaches to itself at d2 = 0.  A free row with no such leader is an ORPHAN (orphans): it lies within jd of an earlier non-leader
 * only, and a later call picks it up.
 * One observation a scan a leader: among the rows of one scan attached to the same leader the one of lowest (d2 bits, row) is
 * kept; the others count in `duplicates`.  k[l] is the number kept: the number of distinct scans that saw l.
 * Confirmation: l is confirmed iff k[l] >= min_obs.  The kept rows of unconfirmed leaders count in `weak`.
 * Ids: first_id = header.n_needed as the call finds it.  The confirmed leaders, in ascending leader row, get first_id, first_id +
 * 1, ...  An id is stored iff it is below the map's max_landmarks; fx_map_update's rule applies to the others: they are counted in
 * n_needed and in not_stored, FX_MAP_FULL is set, their kept rows report -1 and count in `lost`.  `created` counts the stored ids,
 * `added` the kept rows of stored ids.  unmatched = known + free_rows, and free_rows = orphans + duplicates + weak + added + lost.
 * Record of a stored id: fx_map_update's clause for a new landmark: the sums start at 0, the anchor is the (wx, wy) of its first
 * kept row, which is the leader, and every kept row is added in ascending row by "Adding an observation", one fp64 chain on one
 * lane.  n_obs = k; x, y, z and rms_xy by the "Records" clause; first_scan = last_scan = header.scans - 1 (0 when header.scans is
 * 0): the end of the mapping run, the map's "now"; segment = seg; flags = FX_MAP_LM_DISCOVERED; alias stays -1.
 * Header: n_needed += the number of confirmed leaders, n_landmarks = min(n_needed, max_landmarks), n_obs += added, FX_MAP_FULL is
 * set when not_stored > 0.  Nothing else changes: the carry, the carry scan and every existing record, sum and alias entry keep
 * their bytes.
 * Outputs, every word written in both modes: new_id_of_row[r], all q_max_rows words: the stored id for a kept row of a stored
 * landmark, else -1; result: sixteen words, reserved = 0, 0.
 * FX_DISC_DRY_RUN: both outputs are what the applying call would write, and the map is bit for bit what it was.
 * FX_ERR_INVALID_ARG with the reason in fx_last_error(), nothing launched, no output byte touched, the map unchanged: a NULL ctx,
 * map, kp_block_device or loc_device; a NULL map_id_of_row_device with q_max_rows != 0; a map of another context; n_scans == 0 or
 * n_scans > max_scans; known_dist or join_dist not finite and positive; (double)known_dist < 2.0 (double)join_dist; min_obs == 0;
 * unknown require_flags bits; segment == FX_LOC_ANY_SEGMENT; mode > 1; reserved != 0; a keypoint block not 16-byte, records not
 * 8-byte, word arrays not 4-byte aligned.
 * Why known_dist >= 2 join_dist: every kept row lies within jd of its leader and so does the landmark's mean, so a kept row lies
 * within 2 jd of the landmark: a second call on the same inputs finds those rows known and creates no twin.
 * The same bytes from run to run and with any number of contexts in flight: every decision is an integer or a minimum over a total
 * order (32-bit integer atomics only, sums), every fp64 sum an ordered chain on one lane; no floating-point atomics anywhere, and
 * the search structures (two hashed grids, fx_map_merge's, with the cell edges known_dist (1 + 2^-8) over the landmarks and
 * join_dist (1 + 2^-8) over the free rows) never show in a byte.
 * The defaults are choices, not measurements: 0.30 is inlier_dist / merge_dist, and 1.0 m is a little over 2 join_dist twice.
 * Limits: a pole must appear in min_obs scans of ONE call: a caller that hands over a scan a call discovers nothing with the
 * default.  A new pole closer than known_dist to a live landmark of the segment is never discovered.  Discovered landmarks share
 * one scan number: fx_map_merge therefore never joins two of them, and fx_map_close_loop moves them with the loop's end.  Feeding
 * the same scans through fx_map_update as well counts them twice.  A crowded cell is walked by one lane a row: time, not the
 * result, grows with the square of a cell's population.  New in 0.7 (added symbols only). */
#define FX_MAP_LM_DISCOVERED 0x10u   /* fx_map_landmark flags: created by fx_map_discover */
#define FX_DISC_APPLY 0u
#define FX_DISC_DRY_RUN 1u           /* report everything, change no byte of the map */
typedef struct fx_map_discover_options {   /* 32 B */
  float known_dist;       /* a row this close (xy) to a live landmark of the segment is explained; finite, > 0; default 1.0 */
  float join_dist;        /* rows of one new pole lie within this of its leader; finite, > 0; default 0.30 */
  uint32_t min_obs;       /* distinct scans a new pole needs within this call; >= 1; default 3 */
  uint32_t require_flags; /* as fx_map_observe; default FX_LOC_VALID */
  uint32_t segment;       /* a global segment number or FX_LOC_LAST_SEGMENT (default); FX_LOC_ANY_SEGMENT is refused */
  uint32_t mode;          /* FX_DISC_APPLY (default), FX_DISC_DRY_RUN */
  uint32_t reserved[2];   /* 0 */
} fx_map_discover_options;
typedef struct fx_map_discover_result {    /* 64 B */
  uint32_t scans_used, unmatched, known, free_rows, leaders, orphans, duplicates, weak,
           added, lost, created, not_stored, first_id, refused, reserved[2];
} fx_map_discover_result;
void fx_map_discover_options_default(fx_map_discover_options *o);
fx_status fx_map_discover(fx_ctx *ctx, fx_map *map,
    const void *kp_block_device, uint32_t max_scans, uint32_t max_total_keypoints,   /* what the localise was given */
    const fx_localization *loc_device, uint32_t n_scans,                            /* what it wrote */
    const int32_t *map_id_of_row_device, uint32_t q_max_rows,
    const fx_map_discover_options *opt /* NULL: defaults */, fx_map_discover_result *result_device /* or NULL */,
    int32_t *new_id_of_row_device /* [q_max_rows] or NULL */);

/* ---- Compacting the map: the absorbed fragments and the let-go landmarks taken out, the others renumbered ----
 * fx_map_merge leaves every absorbed fragment in place: its record, its sums and its alias entry; every grid build marks and skips
 * them, n_needed only rises, and a map that has filled with them drops new poles for good.  fx_map_compact gives the room back.  It
 * is enqueued on the context's stream (no host synchronisation, no allocation in the steady state: its scratch is the context-owned
 * buffer fx_map_merge uses, which grows once to the map's max_landmarks), may be called between any two other calls on the map, and
 * moves bytes only: no floating-point operation occurs.  fx_map_get's and fx_map_get_alias's addresses stay what they were.
 * ONE CALL, with N = header.n_landmarks and the state as it is when the call runs on the stream:
 * Kept: landmark i < N is kept iff alias[i] == -1 and at least one of: n_obs >= min_obs; (header.scans - 1) - last_scan <
 * min_age_scans in uint32 arithmetic (it was seen lately: it may still grow or be merged); some carry[j], j < header.carry_rows,
 * resolves to i (carry[j] == i, or alias[carry[j]] == i: the next fx_map_update continues it).  Every other landmark is DROPPED: an
 * absorbed one always (its observations live in its root), a live one of few observations not seen for min_age_scans scans when
 * the caller asks for that with min_obs > 1.  With the defaults nothing live is dropped.
 * New ids: a kept landmark's new id is the number of kept landmarks of lower old id (an exclusive prefix: ids stay the order of
 * appearance, and every (distance, id) tie of fx_map_merge and fx_map_localize falls as before).  K = the number kept.
 * Move: a kept landmark's 48-byte record (its FX_MAP_LM_* flags included) and its 8 accumulator doubles go to its new id byte for
 * byte.  alias[0, max_landmarks) becomes -1.  Records and sums at [K, max_landmarks) are unspecified, as after fx_map_reset.
 * Carry: every carry[j] >= 0, j < header.carry_rows, becomes the new id of its resolved root (alias[id] >= 0 ? alias[id] : id),
 * which the rule above keeps; a word beyond N is written as -1.  The carry scan's rows and carry_rows are untouched: an
 * overlap accepted after a compaction continues exactly the landmark it would have continued.
 * header: n_landmarks = n_needed = K; n_obs is reduced by the sum of n_obs over the dropped LIVE landmarks (an absorbed one moved
 * its observations to its root already); scans, batches, segments, flags, carry_rows, last_joined, last_new and last_pose are
 * untouched.  FX_MAP_FULL stays (sticky): room shows as n_landmarks < max_landmarks, and the next new landmark gets the id K.
 * remap (when given), all max_landmarks words: the new id of a kept landmark; the new id of its root for an absorbed one whose
 * root is kept; -1 for everything else, ids >= N included.  A map_id_of_row array of an earlier batch is brought up to date by
 * id = id >= 0 ? remap[id] : -1 alone: no alias lookup is needed.
 * result (when given): before = N, kept = K, dropped_absorbed and dropped_live the two kinds of dropped landmarks.
 * A map with nothing to drop is left bit for bit as it was, with remap[i] = i for i < N (but n_needed of a map that overflowed:
 * it becomes n_landmarks).  A second call changes no byte.  The same bytes from run to run and with any number of contexts in
 * flight: every decision is an integer prefix or a 32-bit sum.
 * FX_ERR_INVALID_ARG with the reason in fx_last_error(), nothing launched, the map unchanged: a NULL ctx or map, a map of another
 * context, min_obs == 0, remap_device or result_device not 4-byte aligned.
 *
 * The snapshot: the map's whole state (private sums, anchors, alias and carry tables and the carry scan included) as one block of
 * host bytes, for a file or for another context on any device.  Little endian; every section starts 16-byte aligned and is zero
 * padded to the next; sections are sized by content, with n = header.n_landmarks and r = header.carry_rows:
 *   block header, 64 B: u32 magic 0x504D5846 ("FXMP"), u32 format 1, u32 fx_version(), u32 64 (this header's size), u32 n, u32 r,
 *     u32 sizeof(fx_map_header) 88, u32 sizeof(fx_map_landmark) 48, u32 8 (accumulator doubles a landmark), u32 0, u64 total bytes,
 *     16 B of zeros
 *   the fx_map_header (88 B -> 96); records[n]; acc[n][8] doubles (Sx, Sy, Sz, ax, ay, Dx, Dy, Q of fx_map_update); alias[n] int32;
 *   carry[r] int32; carry_kp[r], four words a row.
 * The update's state words between launches are 0 between calls and not part of it.
 * fx_map_export_host waits for the stream.  dst_host == NULL with capacity == 0 reports the size in *bytes_out and returns FX_OK; a
 * capacity below the size returns FX_ERR_TOO_LARGE with the size reported and writes nothing; bytes_out may be NULL.  Only the n-
 * and r-prefixes cross the link.
 * fx_map_snapshot_check is host only and needs no device.  FX_ERR_INVALID_ARG with the reason in fx_last_error() when one of these
 * fails: the magic, the format, the block header's size and the three struct sizes, the total against `bytes` and against the sum
 * of the sections; n == the block's header.n_landmarks and r == its header.carry_rows; n_landmarks <= n_needed; every alias word in
 * [-1, n) and fully resolved (alias[alias[i]] == -1); every carry word in [-1, n).  FX_ERR_TOO_LARGE when n > max_landmarks or r >
 * max_carry_rows.  A block with n_needed > n_landmarks (the map overflowed) is refused (FX_ERR_INVALID_ARG) unless max_landmarks
 * == n_landmarks: in a larger map the next landmark would be numbered past a hole; fx_map_compact first, which sets n_needed =
 * n_landmarks.
 * fx_map_import_host runs the check against the target's max_landmarks and max_carry_rows; on failure the target is bit for bit
 * unchanged and nothing is enqueued.  On success it enqueues, on the stream, a reset (alias -1, state words 0) and the copies of
 * the sections; the bytes are staged in context-owned pinned memory before the call returns, so src_host may be freed at once.
 * Afterwards every call (fx_map_update with overlap, merge, localize, compact, export) behaves bit for bit as on the source map;
 * the target may be larger than the source and may live on another context or device.  The import REPLACES the target; to keep
 * the target's landmarks and add the snapshot's behind them use fx_map_append_host (below).  Export and import also return
 * FX_ERR_INVALID_ARG for a NULL ctx, map or src_host, dst_host == NULL with capacity != 0, and a map of another context.  New in
 * 0.7 (added symbols only).
 * Limits: fx_map_compact drops a live landmark only for being short and old; one that stood long and has since gone passes both
 * tests for ever.  fx_map_retire (below) runs this same compaction with the landmarks taken out that fx_map_expect's counts
 * condemn. */
typedef struct fx_map_compact_options {
  uint32_t min_obs;        /* a live landmark of fewer observations may be dropped (see above); >= 1; default 1: drop nothing live */
  uint32_t min_age_scans;  /* ... but only when it was last seen at least this many scans ago; default 64 (fx_map_merge's max_gap_scans) */
} fx_map_compact_options;
typedef struct fx_map_compact_result { uint32_t before, kept, dropped_absorbed, dropped_live; } fx_map_compact_result; /* 16 B */
void fx_map_compact_options_default(fx_map_compact_options *o);
fx_status fx_map_compact(fx_ctx *ctx, fx_map *map, const fx_map_compact_options *opt /* NULL: defaults */,
                         int32_t *remap_device /* [max_landmarks] or NULL */, fx_map_compact_result *result_device /* or NULL */);
fx_status fx_map_export_host(fx_ctx *ctx, fx_map *map, void *dst_host, size_t capacity, size_t *bytes_out);
fx_status fx_map_import_host(fx_ctx *ctx, fx_map *map, const void *src_host, size_t bytes);
fx_status fx_map_snapshot_check(const void *src_host, size_t bytes, uint32_t max_landmarks, uint32_t max_carry_rows); /* Host only */

/* ---- Retiring landmarks on evidence: the ones fx_map_expect's counters condemn taken out of the map ----
 * fx_map_retire reads the two counter arrays the caller accumulated with fx_map_expect (FX_EXPECT_ADD over many localised calls),
 * decides which landmarks are expected again and again and never seen, and runs ONE fx_map_compact with those taken out: the same
 * device code, not a copy of it.  Enqueued on the context's stream, no host synchronisation, no allocation in the steady state,
 * integer operations and byte moves only.  With N = header.n_landmarks and the state as it is when the call runs on the stream:
 * Retired: landmark i < N is retired iff all of: alias[i] == -1; expected[i] >= min_expected; (uint64)seen[i] seen_den <
 * (uint64)expected[i] seen_num (seen / expected < seen_num / seen_den, exactly); no carry[j], j < header.carry_rows, resolves to i
 * (fx_map_compact's clause: the next fx_map_update continues it).
 * Protected: a landmark that meets the first three but is held by the carry counts in protected_by_carry and stays.
 * Then one compaction: fx_map_compact's clauses word for word with min_obs = 1 (and its default min_age_scans), where "kept"
 * additionally requires "not retired": no other live landmark is dropped (every live landmark has n_obs >= 1), and every absorbed
 * one is.  New ids, Move, alias, Carry, header and remap are exactly as there: header.n_obs falls by the n_obs of the retired,
 * remap of a retired landmark (and of an absorbed one whose root is retired) is -1, FX_MAP_FULL stays sticky.
 * Counters follow the landmarks: for a kept i, expected[new id] = expected[i] and seen[new id] = seen[i] (staged through the
 * scratch as the records are: new ids are never above old ones, but the move is parallel); words [K, max_landmarks) become 0.
 * result (when given), 32 B: before = N, kept = K, dropped_absorbed, retired, retired_obs = the sum of n_obs over the retired (in
 * uint32), protected_by_carry, reserved = 0, 0.  retired_of_landmark (when given), all max_landmarks bytes: 1 for a retired OLD id,
 * else 0.
 * FX_RETIRE_DRY_RUN: remap, the byte mask and the result are what the applying call would write; the map and both counter arrays
 * keep every byte.
 * A call in which nothing is retired leaves the map, and remap, byte for byte what fx_map_compact with {min_obs 1} leaves.  A second
 * call changes no byte.  The same bytes from run to run and with any number of contexts in flight.
 * FX_ERR_INVALID_ARG with the reason in fx_last_error(), nothing launched, nothing touched: a NULL ctx, map or counter array; a map
 * of another context; min_expected == 0; seen_den == 0, seen_num == 0 or seen_num > seen_den; mode > 1; reserved != 0; the
 * counters, remap_device or result_device not 4-byte aligned.
 * Limits: the counters of dropped landmarks, absorbed ones included, are discarded: what fx_map_expect counted on an absorbed id
 * before the merge does not pass to its root (expect follows the alias table from the merge on).  The call knows nothing of why a
 * landmark was not seen: occlusion by things that are no keypoints lowers seen / expected of a pole that still stands, and the
 * ratio and min_expected are the caller's guard against that.  New in 0.7 (added symbols only). */
#define FX_RETIRE_APPLY 0u
#define FX_RETIRE_DRY_RUN 1u      /* report everything, change no byte of the map or of the counters */
typedef struct fx_map_retire_options {    /* 24 B */
  uint32_t min_expected;       /* a landmark expected fewer times is never retired; >= 1; default 16 */
  uint32_t seen_num, seen_den; /* retired when seen / expected < seen_num / seen_den; 1 <= num <= den; default 1 / 8 */
  uint32_t mode;               /* FX_RETIRE_APPLY (default), FX_RETIRE_DRY_RUN */
  uint32_t reserved[2];        /* 0 */
} fx_map_retire_options;
typedef struct fx_map_retire_result {     /* 32 B */
  uint32_t before, kept, dropped_absorbed, retired, retired_obs, protected_by_carry, reserved[2];
} fx_map_retire_result;
void fx_map_retire_options_default(fx_map_retire_options *o);
fx_status fx_map_retire(fx_ctx *ctx, fx_map *map,
    uint32_t *expected_of_landmark_device, uint32_t *seen_of_landmark_device,   /* [max_landmarks], read and renumbered */
    const fx_map_retire_options *opt /* NULL: defaults */, int32_t *remap_device /* [max_landmarks] or NULL */,
    uint8_t *retired_of_landmark_device /* [max_landmarks], old ids, or NULL */, fx_map_retire_result *result_device /* or NULL */);

/* ---- Appending one map to another: two maps in two frames become one map with two sets of segments ----
 * Every call above works on ONE map; fx_map_import_host replaces its target and fx_map_update grows a map only from the run it is
 * fed.  fx_map_append puts a second, finished map (another vehicle's, another session's, another rank's, or an old map a live run
 * adopts) behind the first: `dst` afterwards is what it would have been had the source's run been FED to it, its batches through
 * fx_map_update, the first of them without FX_MAP_OVERLAP.  For a source that was only updated this holds bit for bit (it is
 * fx_map_update's own promise that the cut of a run into batches does not show); once the source has been merged, joined or closed
 * the clauses below are the definition.  Both calls are enqueued on the context's stream: no host synchronisation, no allocation in
 * the steady state (the scratch is the context-owned buffer fx_map_merge uses, grown as needed).  No floating-point operation
 * occurs: records and sums move as bytes and only integers are patched, as in fx_map_compact.  The source is only read and every
 * byte of it stays; dst's addresses (fx_map_get, fx_map_get_alias) stay what they were.
 * ONE CALL, with the two maps as they are when the call runs on the stream.  N, Sd and Gd are dst's header.n_landmarks, scans and
 * segments; M and r are the source's header.n_landmarks and carry_rows.
 * Refusals on the device, each of which leaves dst bit for bit unchanged and reports its flag (more than one may be set),
 * appended = 0 and the three bases as they would have been:
 *   FX_APPEND_EMPTY       the source's header.scans == 0: there is no run to append.
 *   FX_APPEND_OVERFLOWED  n_needed > n_landmarks in either map: ids would be numbered past a hole (the snapshot check's reason);
 *                         fx_map_compact first.
 *   FX_APPEND_NO_ROOM     N + M > dst's max_landmarks, in uint64.
 *   FX_APPEND_TOO_LONG    the two maps' scans, segments, batches or n_obs sum to more than 2^32 - 1, in uint64.
 * Otherwise FX_APPEND_APPLIED:
 * Landmarks: the source's landmark i goes to id N + i.  Its 48-byte record and its 8 accumulator doubles are copied byte for byte
 * except three integer fields: first_scan += Sd, last_scan += Sd, segment += Gd.  Its flags, n_obs, doubles and rms_xy keep their
 * bits.  alias[N + i] = the source's alias[i] >= 0 ? alias[i] + N : -1.  Every landmark and every alias word of dst below N keeps
 * every byte.
 * Carry: when r <= dst's max_carry_rows, carry[j] = the source's carry[j] >= 0 ? carry[j] + N : -1 for j < r, the carry scan's
 * rows are the source's and carry_rows = r.  Otherwise carry_rows = 0 and FX_APPEND_CARRY_DROPPED is set: fx_map_update's own rule
 * for a last scan that does not fit.  dst's former carry is gone either way: its run has ended.
 * header: n_landmarks = n_needed = N + M; n_obs, scans, batches and segments are the sums of the two maps' values; flags is the OR
 * of the two maps' flags; last_joined, last_new and last_pose are the source's.
 * result (when given), 32 B: id_base = N, scan_base = Sd, segment_base = Gd, appended = M (0 on a refusal), flags = FX_APPEND_*,
 * carry_rows = dst's header.carry_rows after the call, two reserved words 0.  A caller adds the bases to the ids, global scan
 * numbers and segment labels the source handed out earlier: map_id_of_row arrays, first_global_scan of
 * fx_map_loop_correct_poses, opt.segment.
 * FX_ERR_INVALID_ARG with the reason in fx_last_error(), nothing launched, no byte touched: a NULL ctx, dst, src or src_host;
 * dst == src; a map of another context (for another context or device go through the snapshot); result_device not 4-byte aligned.
 * fx_map_append_host takes the source as a snapshot (fx_map_export_host's bytes).  It runs fx_map_snapshot_check against dst's
 * max_landmarks with no bound on the carry rows and passes its status on; then it stages the bytes in the context's pinned staging
 * as fx_map_import_host does (src_host may be freed at once), copies them into the scratch on the stream and runs the same launch
 * set on the staged sections: one definition and one set of kernels serve both entry points.
 * Limits: nothing is re-framed.  The source's landmarks stay in the source's frame under new segment labels; to bring them into
 * dst's frame: fx_map_find_loop (segment = a source label + segment_base, target_segment = a dst label, recent_scans =
 * 0xffffffff: every landmark of the segment is a query), fx_map_join_segments with prior_device = the find's result,
 * fx_map_merge with a max_gap_scans that covers both runs, fx_map_compact.  After the call the live run is the source's: its next
 * fx_map_update with FX_MAP_OVERLAP is accepted and continues its landmarks under their new ids.  New in 0.7 (added symbols only). */
#define FX_APPEND_APPLIED 0x1u        /* dst was changed: the source's landmarks, carry and counts are in it */
#define FX_APPEND_CARRY_DROPPED 0x2u  /* applied, but the source's carry scan has more rows than dst's max_carry_rows: carry_rows = 0 */
#define FX_APPEND_EMPTY 0x4u          /* refused: the source has seen no scan */
#define FX_APPEND_OVERFLOWED 0x8u     /* refused: n_needed > n_landmarks in one of the maps */
#define FX_APPEND_NO_ROOM 0x10u       /* refused: N + M > dst's max_landmarks */
#define FX_APPEND_TOO_LONG 0x20u      /* refused: a 32-bit count of the header would wrap */
typedef struct fx_map_append_result {  /* 32 B */
  uint32_t id_base, scan_base, segment_base, appended, flags, carry_rows, reserved[2];
} fx_map_append_result;
fx_status fx_map_append(fx_ctx *ctx, fx_map *dst, fx_map *src, fx_map_append_result *result_device /* or NULL */);
fx_status fx_map_append_host(fx_ctx *ctx, fx_map *dst, const void *src_host, size_t bytes,
                             fx_map_append_result *result_device /* or NULL */);

/* ---- Joining two segments of the map: one frame again after a bad link ----
 * fx_track_landmarks holds the pose over an unusable link and starts a new segment; fx_map_update numbers it globally, and from
 * there on the map is two maps in two frames: fx_map_merge merges within a segment, fx_map_localize looks at one segment, and the
 * snapshot carries the split to the next run.  fx_map_join_segments brings the landmarks of segment src into the frame of
 * segment dst and gives both one label: it associates src's landmarks with dst's under a PRIOR transform, fits the correction
 * with fx_map_localize's consensus, moves src's sums, anchors and records, and renumbers the segments.  It is enqueued on the
 * context's stream (no host synchronisation, no allocation in the steady state: its scratch is the context-owned buffer the
 * other map calls share, grown as needed).  Every floating-point step is fp64, no contraction, no fma.
 * Prior: prior_host (c, s, tx, ty, tz; segment and flags are ignored), or prior_device, five doubles c, s, tx, ty, tz read on
 * the device when the call runs (the address of an fx_localization's dc, so that localise-then-join needs no host read), or
 * neither: the identity.  After ONE bad link the held pose leaves src's frame within one link's motion of dst's, which
 * search_dist covers.  The prior takes src's frame to dst's.
 * ONE CALL, with N = header.n_landmarks and SEG = header.segments as they are when the call runs on the stream:
 * Device refusals: src_segment >= SEG or dst_segment >= SEG gives FX_JOIN_BAD_SEGMENT, a prior_device with a double that is
 * not finite FX_JOIN_BAD_PRIOR (both may be set).  The map is bit for bit unchanged; the result is T = the prior's five doubles
 * as they are, D = the identity (dc = 1, ds = dtx = dty = dtz = 0), rms = +inf, n_src = n_corr = n_inliers = moved = 0, label =
 * hyp_a = hyp_b = 0xffffffff, segments = SEG, and every word of match_of_landmark is -1.
 * Targets: g < N is a target iff alias[g] == -1, n_obs >= min_landmark_obs, its x, y and z are finite and segment == dst:
 * fx_map_localize's eligibility clause.
 * Queries: i < N under the same test with segment == src, in ascending id; n_src is their number.  The point of a query is its
 * record under the prior (pc, ps, ptx, pty, ptz): wx = (pc x - ps y) + ptx, wy = (ps x + pc y) + pty, wz = z + ptz.
 * Association: fx_map_localize's clause word for word with the query's point for the row's: dx = x[g] - wx, dy = y[g] - wy, d2 =
 * dx dx + dy dy; g is in reach iff d2 <= sd sd, sd = (double)search_dist; the target of a query is the one in reach of lowest
 * (d2 as uint64 bits, id).  Several queries may pick the same target.
 * Correspondences: the queries that have a target, in ascending id; the first FX_JOIN_MAX_CORR are used (FX_JOIN_TRUNCATED when
 * there are more); n_corr is the number used.  Correspondence k carries q = (wx, wy, wz) and t = (x, y, z) of its target.
 * Hypothesis stage and refit: fx_map_localize's clauses word for word (the same device code) with the query's id in the place of
 * the row: the pool is the H = min(n_corr, hyp_corr) correspondences of lowest (d2 bits, query id).  Without a hypothesis:
 * FX_JOIN_NO_HYPOTHESIS, D = the identity, rms = +inf, n_inliers = 0, hyp_a = hyp_b = 0xffffffff.  Otherwise (dc, ds, dtx, dty,
 * dtz), rms and n_inliers are the final fit, hyp_a and hyp_b the query ids of the winning sample, and FX_JOIN_FITTED is set
 * iff n_inliers >= min_inliers.
 * Transform: with FX_JOIN_FITTED, T = D o prior by fx_map_localize's Pose clause: c = dc pc - ds ps, s = ds pc + dc ps, tx =
 * (dc ptx - ds pty) + dtx, ty = (ds ptx + dc pty) + dty, tz = ptz + dtz.  Otherwise T is the prior's five doubles, bit for bit; D
 * is reported all the same.  mode FX_JOIN_GIVEN skips association and fit: T = the prior, D = the identity, rms = +inf, n_src =
 * n_corr = n_inliers = 0, hyp_a = hyp_b = 0xffffffff.
 * match_of_landmark (when given): all max_landmarks words are written; word i is the target of query i when i is in the final
 * inlier set, -1 everywhere else.
 * Apply: the map is changed iff mode == FX_JOIN_GIVEN, or mode == FX_JOIN_FIT and FX_JOIN_FITTED holds; FX_JOIN_APPLIED is then
 * set.  FX_JOIN_DRY_RUN fits and reports and changes no byte of the map.  Without FX_JOIN_APPLIED moved = 0, label = 0xffffffff,
 * segments = SEG and the map is bit for bit unchanged.  With it:
 *   moved = the number of landmarks i < N with segment == src, absorbed ones included (their frozen records and sums move with
 *   the rest, so the snapshot stays consistent).  For each of them, with n = (double)n_obs and the sums of fx_map_update:
 *   Sx' = (c Sx - s Sy) + n tx, Sy' = (s Sx + c Sy) + n ty, Sz' = Sz + n tz; ax' = (c ax - s ay) + tx, ay' = (s ax + c ay) + ty;
 *   Dx' = c Dx - s Dy, Dy' = s Dx + c Dy; Q is unchanged.  Then its x, y, z and rms_xy are recomputed from the new sums by
 *   fx_map_update's "Records" clause (a landmark of n_obs == 0, which no update makes, keeps its record).  Every landmark reads
 *   and writes its own slot only.
 *   Labels: with lo = min(src, dst) and hi = max(src, dst), every i < N gets segment' = hi - 1 when segment == lo, segment - 1
 *   when segment > lo, segment otherwise; header.segments = SEG - 1; label = hi - 1.  The joined segment keeps the later label
 *   and labels stay dense: when the run's current segment (SEG - 1) takes part it is segments - 1 afterwards, and the next
 *   accepted overlap numbers its new landmarks into the joined segment.  A caller that holds segment numbers from before the
 *   call (an fx_relocalization's pose.segment, an opt.segment) renumbers them by the same rule.
 *   last_pose: iff SEG - 1 == src, its five doubles become T o last_pose by the composition above (p = T, r = last_pose); its
 *   segment and flags stay.  Every other header word, the carry, the carry scan and the alias table stay; ids do not change.
 * result (when given): T, D, rms, n_src, n_corr, n_inliers, flags, moved, label, segments = header.segments after the call,
 * hyp_a, hyp_b.
 * Order of calls: join between an fx_map_update and the next fx_track_landmarks, and read last_pose afterwards for its
 * init_pose_host: the track then continues in dst's frame.
 * FX_ERR_INVALID_ARG with the reason in fx_last_error(), nothing launched, no byte touched: a NULL ctx or map, a map of another
 * context, src_segment == dst_segment, both prior pointers given, a prior_host whose c, s, tx, ty or tz is not finite,
 * search_dist, inlier_dist or min_baseline not finite and positive, hyp_corr outside 2..128, min_inliers < 2, min_landmark_obs
 * == 0, mode > 2, reserved != 0, prior_device or result_device not 8-byte aligned, match_of_landmark_device not 4-byte aligned.
 * The same bytes from run to run and with any number of contexts in flight: every decision is an integer (an integer prefix,
 * 32-bit integer sums) or a minimum over a total order, every fp64 value an ordered chain on one lane.  The search structure
 * (fx_map_merge's hashed grid, cell edge sd (1 + 2^-8)) never shows in a byte; numpy float64 reproduces the call bit for bit.
 * Limits: the duplicates of one pole now share a segment and are fx_map_merge's to join; they are disjoint in time across the
 * cut, and a caller that closes a long loop (fx_map_close_loop, below) raises max_gap_scans.  Q is kept, so rms_xy is exact only for c c + s s = 1 (a
 * fitted or composed T is that within rounding).  One call makes one join.  There is no pose graph: the poses and
 * map_id_of_row arrays handed out earlier are not revised (fx_map_loop_correct_poses, below, revises poses after a loop closure).  New in 0.7 (added symbols only). */
#define FX_JOIN_MAX_CORR 1024u
#define FX_JOIN_FIT 0u      /* mode: fit T from the two segments' landmarks under the prior, apply it */
#define FX_JOIN_GIVEN 1u    /* apply the prior as T, fit nothing */
#define FX_JOIN_DRY_RUN 2u  /* fit and report, change no byte of the map */
typedef struct fx_map_join_options {   /* 32 B */
  float search_dist;      /* as fx_localize_options; default 2.0 */
  float inlier_dist;      /* default 0.30 */
  float min_baseline;     /* default 2.0 */
  uint32_t hyp_corr;      /* 2..128, default 64 */
  uint32_t min_inliers;   /* >= 2, default 3 */
  uint32_t min_landmark_obs; /* >= 1, default 2 */
  uint32_t mode;          /* FX_JOIN_FIT (default), FX_JOIN_GIVEN, FX_JOIN_DRY_RUN */
  uint32_t reserved;      /* 0 */
} fx_map_join_options;
#define FX_JOIN_APPLIED 0x1u        /* the map was changed: src's landmarks moved by T, the segments renumbered */
#define FX_JOIN_TRUNCATED 0x2u      /* more than FX_JOIN_MAX_CORR correspondences: the first 1024 in id order were used */
#define FX_JOIN_NO_HYPOTHESIS 0x4u  /* fewer than 2 correspondences, or no sample passed the gates */
#define FX_JOIN_BAD_PRIOR 0x8u      /* a double of prior_device is not finite */
#define FX_JOIN_BAD_SEGMENT 0x10u   /* src_segment or dst_segment is not below header.segments */
#define FX_JOIN_FITTED 0x20u        /* a correction was fitted to >= min_inliers correspondences: T = D o prior */
typedef struct fx_map_join_result {    /* 120 B */
  double c, s, tx, ty, tz;        /* T: src's frame -> dst's frame */
  double dc, ds, dtx, dty, dtz;   /* D: the fitted correction, T = D o prior */
  float rms;
  uint32_t n_src, n_corr, n_inliers, flags, moved, label, segments;
  uint32_t hyp_a, hyp_b;          /* query ids of the winning sample, 0xffffffff: none */
} fx_map_join_result;
void fx_map_join_options_default(fx_map_join_options *o);
fx_status fx_map_join_segments(fx_ctx *ctx, fx_map *map, uint32_t src_segment, uint32_t dst_segment,
    const fx_pose *prior_host /* or NULL */, const double *prior_device /* 5 doubles c, s, tx, ty, tz, or NULL */,
    const fx_map_join_options *opt /* NULL: defaults */, fx_map_join_result *result_device /* or NULL */,
    int32_t *match_of_landmark_device /* [max_landmarks] or NULL */);

/* ---- Closing a loop in the map: drift spread over the scans of the loop ----
 * A vehicle that comes back to a place it mapped long ago holds every pole there twice, the drift of the loop apart and in one
 * segment: beyond fx_map_merge's merge_dist, and fx_map_localize matches the scan to the recent copies only.
 * fx_map_close_loop associates the RECENT landmarks of one segment with its OLD ones under a prior transform, fits the closure T
 * with fx_map_localize's consensus (the association, the correspondences, the hypothesis stage and the refit are
 * fx_map_join_segments's clauses and run the same device code), and moves every landmark of the segment by a part of T that
 * grows linearly with its time from the old end of the loop (nothing) to the recent end (all of T).  fx_map_loop_correct_poses
 * brings poses handed out earlier up to date by the same rule.  Both are enqueued on the context's stream (no host
 * synchronisation, no allocation in the steady state: the scratch is the context-owned buffer the other map calls share, grown
 * as needed).  Every floating-point step is fp64, no contraction, no fma, no transcendental: the interpolated rotation is a
 * normalised lerp.
 * Prior: as fx_map_join_segments (prior_host, or prior_device: five doubles read on the device, or neither: the identity).  It
 * takes the recent end's frame onto the old one's: about the identity after slow drift, an fx_localization's dc of a scan
 * localised against the old landmarks otherwise.
 * ONE CALL, with N = header.n_landmarks, SEG = header.segments and last = header.scans - 1 as they are when the call runs on
 * the stream; seg is opt.segment, FX_LOC_LAST_SEGMENT standing for SEG - 1 as in fx_map_localize:
 * Device refusals: seg >= SEG (a map of no segment included) or header.scans == 0 gives FX_LOOP_BAD_SEGMENT, a prior_device with
 * a double that is not finite FX_LOOP_BAD_PRIOR (both may be set).  The map is bit for bit unchanged; the result is T = the
 * prior's five doubles as they are, D = the identity (dc = 1, ds = dtx = dty = dtz = 0), px = py = 0, rms = +inf, n_query =
 * n_corr = n_inliers = moved = 0, loop_first_scan = loop_last_scan = hyp_a = hyp_b = 0xffffffff, segment = seg (0xffffffff
 * when FX_LOC_LAST_SEGMENT met a map of no segment), and every word of match_of_landmark is -1.
 * Eligible: g < N with alias[g] == -1, n_obs >= min_landmark_obs, x, y and z finite and segment == seg (fx_map_localize's clause).
 * Targets ("old"): the eligible g with (uint64)last_scan + min_loop_scans <= last.
 * Queries ("recent"): the eligible i with (uint64)first_scan + recent_scans >= last, in ascending id; n_query is their number.
 * recent_scans < min_loop_scans, so no landmark is both and every target ended before every query began.  The point of a query
 * is its record under the prior: wx = (pc x - ps y) + ptx, wy = (ps x + pc y) + pty, wz = z + ptz.
 * Association: dx = x[g] - wx, dy = y[g] - wy, d2 = dx dx + dy dy; target g is in reach iff d2 <= sd sd, sd =
 * (double)search_dist; the target of a query is the one in reach of lowest (d2 as uint64 bits, id).
 * Correspondences: the queries that have a target, in ascending id; the first FX_LOOP_MAX_CORR are used (FX_LOOP_TRUNCATED when
 * there are more); n_corr is the number used.
 * Hypothesis stage and refit: fx_map_localize's clauses with the query's id in the place of the row.  Without a hypothesis:
 * FX_LOOP_NO_HYPOTHESIS, D = the identity, rms = +inf, n_inliers = 0, hyp_a = hyp_b = 0xffffffff.  Otherwise D, rms and
 * n_inliers are the final fit, hyp_a and hyp_b the query ids of the winning sample, and FX_LOOP_FITTED is set iff n_inliers >=
 * min_inliers.  With FX_LOOP_FITTED T = D o prior by fx_map_localize's Pose clause (as in the join), otherwise T is the prior's
 * five doubles bit for bit.  match_of_landmark (when given): all max_landmarks words are written; word i is the target of query
 * i when i is in the final inlier set, -1 everywhere else.
 * Loop bounds, with FX_LOOP_FITTED: s0 = loop_first_scan = the largest last_scan of the targets of the final inlier set, s1 =
 * loop_last_scan = the smallest first_scan of its queries: integer reductions, s0 < s1 by the windows.
 * Pivot, with FX_LOOP_FITTED: px and py are the x and the y of the records (NOT under the prior) of the queries of the final
 * inlier set, each summed sequentially in ascending id from 0.0 and divided once by (double)n_inliers.
 * Without FX_LOOP_FITTED s0 = s1 = 0xffffffff and px = py = 0.  mode FX_LOOP_GIVEN skips association and fit: T = the prior, D =
 * the identity, rms = +inf, counts 0, hyp_a = hyp_b = 0xffffffff, and s0, s1, px and py are the options' loop_first_scan,
 * loop_last_scan, pivot_x and pivot_y.
 * Too far: when mode == FX_LOOP_GIVEN or FX_LOOP_FITTED holds, and T's c is not above 0 (a quarter turn or more: no drift),
 * FX_LOOP_TOO_FAR is set and nothing is applied.
 * Weight of a global scan interval [first_scan, last_scan]: with t2 = (uint64)first_scan + last_scan (twice the mid-scan), alpha
 * = 0 when t2 <= 2 s0, 1 when t2 >= 2 s1, else (double)(t2 - 2 s0) / (double)(2 (s1 - s0)) (both integers in uint64).
 * Interpolated transform T_alpha of T = (c, s, tx, ty, tz): alpha == 1 gives T bit for bit, alpha == 0 the identity (nothing is
 * touched); otherwise, in this order,
 *   cu = (1.0 - alpha) + alpha c, su = alpha s, nrm = sqrt(cu cu + su su), ca = cu / nrm, sa = su / nrm;
 *   gx = (c px - s py) + tx, gy = (s px + c py) + ty                       (the pivot under T);
 *   hx = px + alpha (gx - px), hy = py + alpha (gy - py)                   (the pivot moves on a straight line);
 *   txa = hx - (ca px - sa py), tya = hy - (sa px + ca py), tza = alpha tz.
 * Apply: the map is changed iff FX_LOOP_TOO_FAR is not set and either mode == FX_LOOP_GIVEN, or mode == FX_LOOP_FIT and
 * FX_LOOP_FITTED holds; FX_LOOP_APPLIED is then set.  FX_LOOP_DRY_RUN fits and reports and changes no byte.  Without
 * FX_LOOP_APPLIED moved = 0 and the map is bit for bit unchanged.  With it:
 *   every landmark i < N of segment seg whose alpha (of its first_scan and last_scan) is above 0, absorbed ones included (their
 *   frozen records and sums move with the rest), moves its sums, its anchor and its record under its T_alpha by
 *   fx_map_join_segments's Apply formulas with (ca, sa, txa, tya, tza) for (c, s, tx, ty, tz): Q is kept and x, y, z and rms_xy
 *   are recomputed by fx_map_update's "Records" clause (a landmark of n_obs == 0 keeps its record).  moved is their number.
 *   Every landmark reads and writes its own slot only; landmarks of other segments and those with alpha == 0 keep every byte.
 *   last_pose: iff seg == SEG - 1, its five doubles become T_alpha o last_pose (p = T_alpha, r = last_pose in the Pose clause's
 *   composition) with alpha taken at t2 = 2 last (a fitted loop has last >= s1: that is T itself); alpha == 0 leaves it.  Its
 *   segment and flags stay.  Every other header word, the alias table, the carry, the carry scan, ids, labels and n_obs stay.
 * result (when given): T, D, px, py, rms, n_query, n_corr, n_inliers, flags, moved, loop_first_scan, loop_last_scan, segment =
 * seg, hyp_a, hyp_b, reserved = 0.
 * Order of calls: close between an fx_map_update and the next fx_track_landmarks, and read last_pose afterwards for its
 * init_pose_host.  Then fx_map_merge with a max_gap_scans that covers the loop fuses the twins, and fx_map_compact drops them.
 * fx_map_loop_correct_poses: pose b of poses_device is the pose of global scan first_global_scan + b.  When the result carries
 * FX_LOOP_APPLIED and the alpha of t2 = 2 (first_global_scan + b) (uint64) is above 0, the pose's five doubles become T_alpha o
 * pose by the same composition; its segment and flags stay.  Without FX_LOOP_APPLIED nothing is written.  The caller passes
 * only poses of the closed segment (result.segment).  One lane a pose.
 * FX_ERR_INVALID_ARG with the reason in fx_last_error(), nothing launched, no byte touched: a NULL ctx or map, a map of another
 * context, both prior pointers given, a prior_host whose c, s, tx, ty or tz is not finite, search_dist, inlier_dist or
 * min_baseline not finite and positive, hyp_corr outside 2..128, min_inliers < 2, min_landmark_obs == 0, recent_scans >=
 * min_loop_scans, segment == FX_LOC_ANY_SEGMENT, mode > 2, in mode FX_LOOP_GIVEN loop_first_scan >= loop_last_scan or a pivot
 * that is not finite, reserved != 0, prior_device or result_device not 8-byte aligned, match_of_landmark_device not 4-byte
 * aligned; fx_map_loop_correct_poses: a NULL ctx, result or poses, a result or poses not 8-byte aligned.
 * The same bytes from run to run and with any number of contexts in flight: every decision is an integer or a minimum over a
 * total order, every fp64 value an ordered chain of + - * / sqrt on one lane.  The grid never shows in a byte; numpy float64
 * reproduces both calls bit for bit.
 * Limits: a landmark carries two scan numbers, not a trajectory: its weight is that of its mid-scan, so the correction is first
 * order, a linear spread of the closure error over the scans and no pose-graph optimum.  A landmark whose observations already
 * span the loop (one merged across it) is placed by its mid-scan: close before merging across the loop.  Q is kept, so rms_xy is
 * exact only for ca ca + sa sa = 1 (true within rounding).  One call closes one loop.  New in 0.7 (added symbols only). */
#define FX_LOOP_MAX_CORR 1024u
#define FX_LOOP_FIT 0u      /* mode: fit T from the segment's recent and old landmarks under the prior, apply it spread */
#define FX_LOOP_GIVEN 1u    /* apply the prior as T between the given scans about the given pivot, fit nothing */
#define FX_LOOP_DRY_RUN 2u  /* fit and report, change no byte of the map */
typedef struct fx_map_loop_options {   /* 72 B */
  float search_dist;      /* as fx_map_join_options; default 2.0 */
  float inlier_dist;      /* default 0.30 */
  float min_baseline;     /* default 2.0 */
  uint32_t hyp_corr;      /* 2..128, default 64 */
  uint32_t min_inliers;   /* >= 2, default 3 */
  uint32_t min_landmark_obs; /* >= 1, default 2 */
  uint32_t segment;       /* a global segment, or FX_LOC_LAST_SEGMENT (default); FX_LOC_ANY_SEGMENT is refused */
  uint32_t min_loop_scans; /* a target ended at least this many scans before the map's last; default 256 */
  uint32_t recent_scans;  /* a query began at most this many scans before the map's last; < min_loop_scans; default 32 */
  uint32_t mode;          /* FX_LOOP_FIT (default), FX_LOOP_GIVEN, FX_LOOP_DRY_RUN */
  uint32_t loop_first_scan, loop_last_scan; /* FX_LOOP_GIVEN only: s0 < s1; default 0, 0 */
  double pivot_x, pivot_y; /* FX_LOOP_GIVEN only: finite; default 0, 0 */
  uint32_t reserved;      /* 0 */
} fx_map_loop_options;
#define FX_LOOP_APPLIED 0x1u        /* the map was changed: the segment's landmarks moved by their part of T */
#define FX_LOOP_TRUNCATED 0x2u      /* more than FX_LOOP_MAX_CORR correspondences: the first 1024 in id order were used */
#define FX_LOOP_NO_HYPOTHESIS 0x4u  /* fewer than 2 correspondences, or no sample passed the gates */
#define FX_LOOP_BAD_PRIOR 0x8u      /* a double of prior_device is not finite */
#define FX_LOOP_BAD_SEGMENT 0x10u   /* the segment is not below header.segments, or the map has no scans */
#define FX_LOOP_FITTED 0x20u        /* a closure was fitted to >= min_inliers correspondences: T = D o prior */
#define FX_LOOP_TOO_FAR 0x40u       /* T turns by a quarter turn or more: no drift, nothing applied */
typedef struct fx_map_loop_result {    /* 144 B */
  double c, s, tx, ty, tz;        /* T: the recent end of the loop -> the old one */
  double dc, ds, dtx, dty, dtz;   /* D: the fitted correction, T = D o prior */
  double px, py;                  /* the pivot */
  float rms;
  uint32_t n_query, n_corr, n_inliers, flags, moved;
  uint32_t loop_first_scan, loop_last_scan; /* s0, s1; 0xffffffff: none */
  uint32_t segment;               /* the resolved segment */
  uint32_t hyp_a, hyp_b;          /* query ids of the winning sample, 0xffffffff: none */
  uint32_t reserved;              /* 0 */
} fx_map_loop_result;
void fx_map_loop_options_default(fx_map_loop_options *o);
fx_status fx_map_close_loop(fx_ctx *ctx, fx_map *map,
    const fx_pose *prior_host /* or NULL */, const double *prior_device /* 5 doubles c, s, tx, ty, tz, or NULL */,
    const fx_map_loop_options *opt /* NULL: defaults */, fx_map_loop_result *result_device /* or NULL */,
    int32_t *match_of_landmark_device /* [max_landmarks] or NULL */);
fx_status fx_map_loop_correct_poses(fx_ctx *ctx, const fx_map_loop_result *result_device,
    fx_pose *poses_device, uint32_t first_global_scan, uint32_t n_poses);

/* ---- Finding a loop's closure without a prior: the recent landmarks laid on the old ones as a constellation ----
 * fx_map_close_loop and fx_map_join_segments need a prior within search_dist of the truth.  Once the drift of a loop (or the
 * displacement of a segment) is larger, fx_map_localize matches a scan to the recent copies of the poles and fx_map_relocalize
 * sees both copies as rivals of each other.  fx_map_find_loop runs fx_map_relocalize's constellation search on the map's own
 * landmarks with the loop's two time windows: the RECENT landmarks of one segment (the queries) stand in the place of a scan's
 * keypoints, and only the OLD landmarks of that segment, or the landmarks of another segment (the targets), can be landed on.
 * The first 40 bytes of its result are five doubles c, s, tx, ty, tz: what fx_map_close_loop and fx_map_join_segments take as
 * prior_device, so find-then-close and find-then-join need no host read.  It is enqueued on the context's stream (no host
 * synchronisation, no allocation in the steady state: its scratch is the context-owned buffer the other map calls share, grown
 * as needed) and READS the map only: header, records, sums, alias, carry and the carry scan are bit for bit what they were.
 * Every floating-point step is fp64, no contraction, no fma, no transcendental; id, pt, mb, xb are inlier_dist, pair_tol,
 * min_baseline and max_baseline widened to double.
 * ONE CALL, with N = header.n_landmarks, SEG = header.segments and last = header.scans - 1 as they are when the call runs on the
 * stream:
 * Segments: qseg is opt.segment, FX_LOC_LAST_SEGMENT standing for SEG - 1.  tseg is opt.target_segment: FX_FIND_SAME_SEGMENT
 * (the default) stands for qseg, any other value is a global segment number or FX_LOC_LAST_SEGMENT.
 * Device refusal: qseg >= SEG or tseg >= SEG (a map of no segment included), header.scans == 0, or a target_segment other than
 * FX_FIND_SAME_SEGMENT that resolves to qseg, gives flags = FX_FIND_BAD_SEGMENT alone: the record is that of a call without a
 * winner (below) with n_hyp = n_query = n_targets = n_seeds = 0, segment and target_segment the resolved numbers (0xffffffff
 * where FX_LOC_LAST_SEGMENT met a map of no segment), and every word of match_of_landmark is -1.
 * Eligible: fx_map_localize's clause: g < N with alias[g] == -1, n_obs >= min_landmark_obs and x, y and z finite.
 * Targets: the eligible g of segment tseg; when tseg is qseg (FX_FIND_SAME_SEGMENT) they must also be OLD, (uint64)last_scan +
 * min_loop_scans <= last.  n_targets is their number.
 * Queries: the candidates are the eligible i of segment qseg with (uint64)first_scan + recent_scans >= last (recent_scans =
 * 0xffffffff admits the whole segment).  They are taken in DESCENDING id and at most the first FX_FIND_MAX_QUERY are used (more:
 * FX_FIND_TRUNCATED): the youngest landmarks are the ones the vehicle is among.  Query k is the k-th used one in that order,
 * n_query the number used; their coordinates are the records' doubles as they are.  No landmark is both a query and a target
 * (recent_scans < min_loop_scans in one segment; two segments otherwise).
 * Seeds, hypotheses, score: fx_map_relocalize's clauses word for word, query k in the place of keypoint k and the targets in the
 * place of the eligible landmarks: the candidate pairs (a, b), a < b, of queries with mb mb <= d2 <= xb xb, ranked by descending
 * d2 bits, then ascending (a, b), the first n_seeds = min(count, max_seeds) used; for the seed of rank s every ordered pair (g, h),
 * g != h, of targets under the hypothesis clause in fp64 with mb mb as the baseline gate and pt as the length gate; the score of a
 * hypothesis is the number of queries whose image has a target with d2 <= id id.  n_hyp counts the hypotheses.
 * Winner: the hypothesis of highest score, ties to the lowest (s, g, h).  A best score below 2, or no hypothesis, is NO WINNER:
 * flags = FX_FIND_NO_HYPOTHESIS (and FX_FIND_TRUNCATED when it applies), wc = 1, ws = wtx = wty = wtz = 0, score = runner_up = 0,
 * seed_a = seed_b = lm_a = lm_b = 0xffffffff; the counts are what they are.
 * Rivals and runner_up: fx_map_relocalize's clause with g = 2.0 id.
 * With a winner: the target of a query is the target of lowest (d2 as uint64 bits, id) among those with d2 <= id id of its image
 * (the SCORED queries are those that have one); wtz is the sequential sum, in ascending k, of Z[target] - z over the scored
 * queries, divided once by (double)score; wc, ws, wtx, wty are the winner's transform, query frame -> target frame; seed_a,
 * seed_b are the landmark ids of the winning seed's queries and lm_a, lm_b the targets g, h.  FX_FIND_VALID iff score >=
 * min_inliers and score - runner_up >= min_margin; FX_FIND_AMBIGUOUS iff score >= min_inliers and the margin fails; neither below
 * min_inliers.
 * The head: with FX_FIND_VALID c, s, tx, ty, tz = wc, ws, wtx, wty, wtz.  Without it all five are the quiet NaN
 * 0x7ff8000000000000, on purpose: a chained fx_map_close_loop or fx_map_join_segments then answers FX_LOOP_BAD_PRIOR or
 * FX_JOIN_BAD_PRIOR and leaves the map bit for bit, so a loop that was not found can never move the map.
 * match_of_landmark (when given): all max_landmarks words are written; word i is the target of query i for the scored queries of
 * a FX_FIND_VALID result and -1 everywhere else.
 * The chains: fx_map_find_loop, then fx_map_close_loop(NULL, (const double *)result, search_dist about 2 inlier_dist), then
 * fx_map_loop_correct_poses, fx_map_merge and fx_map_compact; or fx_map_find_loop with target_segment = dst and segment = src,
 * then fx_map_join_segments(src, dst, NULL, (const double *)result).
 * FX_ERR_INVALID_ARG with the reason in fx_last_error(), nothing launched, no byte touched: a NULL ctx, map or result, a map of
 * another context, inlier_dist, pair_tol or min_baseline not finite and positive, max_baseline not finite or below min_baseline,
 * max_seeds outside 1..64, min_inliers < 3, min_margin == 0, min_landmark_obs == 0, segment or target_segment ==
 * FX_LOC_ANY_SEGMENT, recent_scans >= min_loop_scans with target_segment == FX_FIND_SAME_SEGMENT, reserved != 0, result_device
 * not 8-byte aligned, match_of_landmark_device not 4-byte aligned.
 * The same bytes from run to run and with any number of contexts in flight: every decision is an integer (32- and 64-bit integer
 * atomics only, sum and maximum) or a minimum over a total order, every fp64 value an ordered chain on one lane.  The two grids
 * (fx_map_relocalize's) and the reduction never show in a result; numpy float64 reproduces the record and match_of_landmark bit
 * for bit.
 * Limits: as fx_map_relocalize: the transform is that of ONE two-point hypothesis, which the chained call refits over all
 * correspondences; poles that repeat a pattern come back AMBIGUOUS; fewer than three twins cannot be VALID.  One call finds one
 * loop.  New in 0.7 (added symbols only). */
#define FX_FIND_MAX_QUERY 64u
#define FX_FIND_SAME_SEGMENT 0xfffffffdu  /* target_segment: the targets are the old landmarks of opt.segment itself */
typedef struct fx_map_find_loop_options {   /* 52 B */
  float inlier_dist;      /* a query lands on a target within this xy distance, m; finite, > 0; default 0.30 */
  float pair_tol;         /* allowed difference between a seed's length and a target pair's; finite, > 0; default 0.30 */
  float min_baseline;     /* shortest seed pair, m; finite, > 0; default 2.0 */
  float max_baseline;     /* longest seed pair, m; finite, >= min_baseline; default 60.0 */
  uint32_t max_seeds;     /* seed pairs tried; 1..64, default 16 */
  uint32_t min_inliers;   /* score needed for FX_FIND_VALID; >= 3, default 4 */
  uint32_t min_margin;    /* lead needed over the best rival; >= 1, default 1 */
  uint32_t min_landmark_obs; /* a landmark takes part with at least this many observations; >= 1, default 2 */
  uint32_t segment;       /* the queries' segment: a global segment, or FX_LOC_LAST_SEGMENT (default); FX_LOC_ANY_SEGMENT is refused */
  uint32_t target_segment; /* FX_FIND_SAME_SEGMENT (default), a global segment other than `segment`, or FX_LOC_LAST_SEGMENT */
  uint32_t min_loop_scans; /* as fx_map_loop_options; ignored when the targets are another segment's; default 256 */
  uint32_t recent_scans;  /* as fx_map_loop_options; < min_loop_scans with FX_FIND_SAME_SEGMENT; default 32 */
  uint32_t reserved;      /* 0 */
} fx_map_find_loop_options;
#define FX_FIND_VALID 0x1u         /* score >= min_inliers and score - runner_up >= min_margin: c, s, tx, ty, tz are the transform */
#define FX_FIND_TRUNCATED 0x2u     /* more than FX_FIND_MAX_QUERY candidate queries: the 64 of highest id were used */
#define FX_FIND_NO_HYPOTHESIS 0x4u /* no hypothesis, or none that lands 2 queries */
#define FX_FIND_AMBIGUOUS 0x8u     /* score >= min_inliers, but a rival transform scores within min_margin of it */
#define FX_FIND_BAD_SEGMENT 0x10u  /* a segment is not below header.segments, the map has no scans, or target_segment names segment */
typedef struct fx_map_loop_candidate {  /* 136 B */
  double c, s, tx, ty, tz;          /* with FX_FIND_VALID the winner's transform, query frame -> target frame; else quiet NaNs */
  double wc, ws, wtx, wty, wtz;     /* the winner's transform whenever there is one (AMBIGUOUS included); else the identity */
  uint64_t n_hyp;                   /* hypotheses counted */
  uint32_t n_query, n_targets, n_seeds, score, runner_up, flags;
  uint32_t seed_a, seed_b;          /* landmark ids of the winning seed's queries, 0xffffffff: none */
  uint32_t lm_a, lm_b;              /* the targets they were laid on, 0xffffffff: none */
  uint32_t segment, target_segment; /* the resolved numbers */
} fx_map_loop_candidate;
void fx_map_find_loop_options_default(fx_map_find_loop_options *o);
fx_status fx_map_find_loop(fx_ctx *ctx, fx_map *map, const fx_map_find_loop_options *opt /* NULL: defaults */,
    fx_map_loop_candidate *result_device, int32_t *match_of_landmark_device /* [max_landmarks] or NULL */);

/* ---- Splicing two batches' blocks: every scan processed once ----
 * fx_map_update continues tracks across a one-scan overlap: batch k + 1 must begin with the scan batch k ended with.  That scan's
 * keypoints are rows of batch k's keypoint block and its descriptors rows of batch k's CSR block, and a scan's result does not
 * depend on its batch (the map's bitwise overlap check rests on that), so the scan need not go through fx_process_batch again.
 * fx_splice_blocks builds one block pair from scans of two existing block pairs: the destination is what fx_pack_keypoint_block
 * and fx_pack_descriptors_csr would write for a batch of exactly those scans.  Match, register, track and fx_map_update run on it
 * unchanged.  Splicing (previous, FX_SPLICE_LAST_SCAN, 1) with (current, 0, all) is the overlap; (previous, 0, all) with
 * (current, 0, all) lays two batches side by side for a match across them.
 * Selection.  For a source X: S = min(its header's scans, max_scans), K = min(its header's keypoints stored,
 * max_total_keypoints).  scan0 == FX_SPLICE_LAST_SCAN stands for S - 1 and selects nothing in a block of no scans.  The selected
 * scans are [scan0, min(scan0 + n_scans, S)), computed without 32-bit wrap: n_scans = 0xffffffff means "to the end", a scan0 at or
 * beyond S selects nothing.  The rows of scan i are [min(kp_offset[i], K), min(kp_offset[i + 1], K)), taken as empty when they do
 * not increase: a block of garbage is memory-safe and gives an unspecified destination.  Every count is read on the device: the
 * call reads nothing on the host and does not synchronise.  a and b may be the same block.
 * The virtual batch is a's selected scans in order, then b's: n scans, each with its rows, its source flag word and its source
 * CSR rows under the same row numbers.  A source CSR row r exists iff r is below that CSR block's rows_stored.
 * Keypoint block: byte for byte what fx_pack_keypoint_block writes for a batch of those n scans under (dst_max_scans,
 * dst_max_total_keypoints).  Row 0 is {min(n, dst_max_scans), total, OR of the written flags, dst_max_total_keypoints}; the
 * offsets are clipped to dst_max_total_keypoints and repeat the total beyond the batch; flags beyond the batch are 0; keypoint
 * rows past the total are zero.  FX_FLAG_KP_OVERFLOW is set on every scan that holds fewer rows in dst than in its source, and
 * in row 0; it is also set in row 0 when n > dst_max_scans.  All fx_keypoint_block_bytes bytes are written.
 * CSR block (dst_csr_block_device, given only together with both sources' CSR blocks): rows is the number of virtual rows of all
 * n scans; as in the pack it is not clipped by dst_max_scans or dst_max_total_keypoints.  Virtual row v is stored iff every row
 * u <= v exists in its source, has u < dst_max_rows and a cumulative end <= dst_capacity.  row_ptr[0] = 0, the ends of the
 * stored rows follow, the entries after them up to dst_max_rows repeat nnz_stored.  nnz_needed is the sum over all virtual rows
 * that exist in their source: a lower bound when a source was itself cut.  col and val of the stored rows are copied bit for bit
 * (-0.0 and any NaN payload included).  Nothing is written at or beyond nnz_stored, or in the sections' padding.
 * FX_ERR_INVALID_ARG with the reason in fx_last_error(), nothing launched, no byte touched: a NULL ctx, source or dst keypoint
 * block; a dst CSR block without both sources' CSR blocks; a block that is not 16-byte aligned; a max_scans of 0; a dst block
 * whose byte range (fx_keypoint_block_bytes / fx_descriptor_csr_bytes of its layout) overlaps a source block's.
 * Enqueued on the context's stream: two launches, no allocation in the steady state (the plan words live in a context-owned
 * scratch that grows), integer operations only, the same bytes from run to run.  New in 0.7 (added symbols only). */
#define FX_SPLICE_LAST_SCAN 0xffffffffu  /* scan0: the source's last scan (scans - 1, read on the device); nothing in a block of no scans */
typedef struct fx_splice_source {
  const void *kp_block_device;  uint32_t max_scans, max_total_keypoints;   /* layout as given to fx_pack_keypoint_block */
  const void *csr_block_device; uint32_t max_rows, capacity;               /* layout as given to fx_pack_descriptors_csr; ignored when the dst CSR is NULL */
  uint32_t scan0, n_scans;                                                 /* scans [scan0, scan0 + n_scans) of this source, clipped */
} fx_splice_source;
fx_status fx_splice_blocks(fx_ctx *ctx, const fx_splice_source *a, const fx_splice_source *b,
    void *dst_kp_block_device, uint32_t dst_max_scans, uint32_t dst_max_total_keypoints,
    void *dst_csr_block_device /* or NULL: keypoints only */, uint32_t dst_max_rows, uint32_t dst_capacity);

/* ---- De-skewing a block's keypoints for the sensor's motion during a sweep ----
 * A spinning sensor captures a scan over a whole sweep while it moves; every call behind fx_process_batch (fx_register_matches,
 * fx_track_landmarks, fx_map_update, fx_map_localize, fx_map_relocalize, fx_map_observe, fx_map_expect, fx_map_discover, the loop
 * calls) reads a scan's keypoints as one rigid snapshot.  All rings fire at one azimuth at nearly the same time, so a pole's
 * clusters, and the keypoint the secondary merge makes of them, are captured within about a millisecond: moving the KEYPOINT by the
 * sensor's motion between its capture and the scan's stamp is, to first order, de-skewing the points.  fx_deskew_keypoint_block
 * does that with the motion over one scan period the caller holds on the device (fx_register_matches's records, or odometry) and
 * writes a block of the same layout, which every call above takes unchanged.  The descriptors (local, R = 2.5 m) stay as they are.
 * Sizes: S = min(n_scans, the block's scans, max_scans), rows = min(the block's keypoints stored, max_total_keypoints); scan(r) and
 * the non-rows exactly as in fx_track_landmarks (csrc/fx_scan_query.h, the one device definition).  The whole block is written:
 * row 0, the kp_offset rows and the flag rows byte for byte, and byte for byte every row of the keypoint area that is not corrected
 * (rows beyond `rows`, non-rows, rows of scans >= S included).  All n_scans records are written and nothing beyond them.
 * Every floating-point step below is fp64, no contraction, no fma, each expression in the stated order.
 * Usable motion: a record is usable iff (flags & require_flags) == require_flags, its c, s, tx, ty and tz are finite, and c > 0
 * (less than a quarter turn a period; it also keeps the interpolation's norm away from 0).
 * The motion of scan b < S: FX_DESKEW_PER_SCAN: record b.  FX_DESKEW_LINKS: record b - 1 (when b >= 1) if usable; otherwise
 * record b (when b + 1 < S) if usable, with FX_DESKEW_NEXT_LINK (constant velocity: the motion into the next scan stands for
 * this one).  With a usable record the scan is FX_DESKEW_MOVED and `motion` its index.  Without: FX_DESKEW_NO_MOTION, motion =
 * 0xffffffff, the scan's rows are copied.  b >= S: FX_DESKEW_NO_SCAN only, motion = 0xffffffff, rows_moved = 0, max_shift = 0.
 * Turn of a row (x, y the floats widened): ax = |x|, ay = |y|, hi = ay > ax ? ay : ax, lo = the other; the turn is 0.0 when hi
 * is not > 0; otherwise a = lo / hi, t = a a, g = a (k0 + t (k1 + t (k2 + t (k3 + t (k4 + t k5))))) with FX_DESKEW_TURN_K's six
 * constants (a least-squares odd polynomial for atan(a) / 2 pi on [0, 1]: within 2.9e-7 of a turn, monotone, a step of 5e-7
 * upwards at the octant seam); q = ay > ax ? 0.25 - g : g; h = x < 0.0 ? 0.5 - q : q; turn = y < 0.0 ? -h : h (-0.0 is not below
 * 0).  No library arctangent: numpy reproduces the turn bit for bit.
 * Sweep fraction: u = (double)direction (turn - start_turn); phi = u - floor(u), taken as 0.0 when that is >= 1.0;
 * a = (phi - ref_fraction) sweep_fraction.
 * Correction of a row of a MOVED scan whose x, y, z are finite (every other row is copied and not counted): w = |a|; w == 0.0
 * copies the row bit for bit.  G = the motion M when a > 0; when a < 0, M's inverse taken as (c, -s, -(c tx + s ty),
 * (s tx - c ty), -tz).  (ca, sa, txa, tya, tza) is fx_map_close_loop's "Interpolated transform" of G with pivot (0, 0) and alpha =
 * w (the same device function; w == 1 gives G bit for bit).  x' = (ca x - sa y) + txa, y' = (sa x + ca y) + tya, z' = z + tza,
 * each rounded once to float; the fourth word (the elevation) is copied bit for bit.
 * Records: rows_moved counts the corrected rows; max_shift is the maximum over them of (float)sqrt(dx dx + dy dy), dx and dy
 * taken in fp64 between the stored floats and the source floats (a 32-bit integer maximum on the bit pattern: order-free).
 * dst may be src itself (in place) or disjoint from it.  motions[p] of FX_DESKEW_LINKS, p < n_scans - 1, is the record "scan
 * p + 1 -> scan p" fx_register_matches wrote for capi.pairs_consecutive; it is read on the device, so a register in front of the
 * call needs no host read.
 * FX_ERR_INVALID_ARG with the reason in fx_last_error(), nothing launched, no output byte touched: a NULL required pointer
 * (motions may be NULL only with FX_DESKEW_LINKS and n_scans == 1; opt NULL = the defaults), n_scans == 0 or n_scans > max_scans,
 * a start_turn that is not finite, ref_fraction outside [0, 1], sweep_fraction outside (0, 1], a direction that is not +1 or -1,
 * an unknown source, reserved != 0, blocks not 16-byte, records not 8-byte or `out` not 4-byte aligned, a dst that overlaps src
 * without being equal to it.
 * Limits: the motion is taken as constant over a period; levelling (roll, pitch) changes a row's azimuth only to second order; a
 * pole at the sweep's seam is ambiguous (with the reference's pass-through box, x >= 0, and the seam behind the sensor none lies
 * there); descriptors are not recomputed; de-skewing the points themselves is out of scope.
 * Enqueued on the context's stream: a memset of the records and one launch, no host synchronisation, no allocation; needs no
 * batch to have been processed.  The same bytes from run to run and with any number of contexts in flight: every decision is an
 * integer or an ordered, correctly rounded operation on one lane, the two reductions are 32-bit integer atomics.  New in 0.7
 * (added symbols only). */
#define FX_DESKEW_LINKS    0u  /* motions[p], p < n_scans - 1, is the link record "scan p + 1 -> scan p" (what fx_register_matches wrote for pairs_consecutive) */
#define FX_DESKEW_PER_SCAN 1u  /* motions[b], b < n_scans, is scan b's own motion over one scan period (odometry, IMU), same meaning of the five doubles */
/* k0 .. k5 of the turn's polynomial: the one place the device reads (csrc/fx_deskew.hip) and capi.DESKEW_TURN_K restates */
#define FX_DESKEW_TURN_K {0.15915173357526405, -0.052943764423474274, 0.030823588143917297, -0.01856560178002491, 0.008407119202664756, -0.001873333241134883}
typedef struct fx_deskew_options {   /* 40 B */
  double start_turn;      /* azimuth where a sweep begins, in turns of atan2(y, x); finite; default 0.5 (behind the sensor) */
  double ref_fraction;    /* the sweep fraction the scan's pose refers to; 0 start .. 1 end; in [0, 1]; default 1.0 */
  double sweep_fraction;  /* share of the scan period that one sweep takes; in (0, 1]; default 1.0 (continuous rotation) */
  int32_t direction;      /* +1: azimuth grows during the sweep, -1: it falls (a Velodyne seen from above; note node.cpp:65's roll - pi flips it); default -1 */
  uint32_t source;        /* FX_DESKEW_LINKS (default) or FX_DESKEW_PER_SCAN */
  uint32_t require_flags; /* FX_REG_* bits a motion record must carry; default FX_REG_VALID */
  uint32_t reserved;      /* 0 */
} fx_deskew_options;
#define FX_DESKEW_MOVED 0x1u      /* a usable motion was found: the scan's finite rows were corrected */
#define FX_DESKEW_NEXT_LINK 0x2u  /* (LINKS) link b - 1 was not usable, link b was taken */
#define FX_DESKEW_NO_MOTION 0x4u  /* no usable motion: the scan's rows are copied bit for bit */
#define FX_DESKEW_NO_SCAN 0x8u    /* b is beyond the block's scans */
typedef struct fx_deskew_scan {   /* 16 B, one per scan */
  uint32_t flags, motion;         /* motion: index of the record used, 0xffffffff: none */
  uint32_t rows_moved;            /* rows written through the correction (w != 0) */
  float max_shift;                /* largest xy distance between a corrected row (as stored) and its source row; 0 when none */
} fx_deskew_scan;
void fx_deskew_options_default(fx_deskew_options *o);
fx_status fx_deskew_keypoint_block(fx_ctx *ctx,
    const void *src_block_device, void *dst_block_device, uint32_t max_scans, uint32_t max_total_keypoints,
    const fx_registration *motions_device, uint32_t n_scans, const fx_deskew_options *opt /* NULL: defaults */,
    fx_deskew_scan *out_device /* [n_scans] */);

/* ---- Following a stream of scans through the map: each scan's fix is the next scan's prior ----
 * fx_map_localize takes one prior a scan and localises the scans of a call in parallel, so a scan's fix never helps the next
 * scan's prior, and dead-reckoned priors (fx_track_landmarks's fold of the links from one start pose) drift out of search_dist.
 * fx_map_follow runs CHAINS of consecutive scans: the prior of scan b is the pose of scan b - 1 (its fix when FX_LOC_VALID,
 * otherwise its own prior) composed with the motion into scan b, and scan b is then localised exactly as fx_map_localize would
 * under that prior.  Many chains run at once, one workgroup each; a chain's only dependence is its own loop.  The call is
 * enqueued on the context's stream, never waits for it, READS the map only (bit for bit what it was) and allocates nothing in the
 * steady state: its scratch is fx_map_localize's carve of the shared buffer.
 * Sizes, non-rows and eligible landmarks: exactly fx_map_localize's, with opt.loc for its options and kp_offset ascending (as
 * fx_pack_keypoint_block writes it).  Chains: L = opt.chain_scans, or n_scans when that is 0; chain j is the scans
 * [j L, min((j + 1) L, n_scans)), n_chains = ceil(n_scans / L); start_poses_device holds n_chains fx_pose records and is read on
 * the device.  links[p], p < n_scans - 1, is the record "scan p + 1 -> scan p" fx_register_matches wrote for pairs_consecutive.
 * For chain j with first scan f, in scan order:
 * 1. Scan f: prior = start_poses[j] bit for bit (all 48 bytes), FX_FOLLOW_START, motion = 0xffffffff.
 * 2. Scan b > f: p* = out[b - 1].pose.  Link b - 1 is usable iff (flags & require_flags) == require_flags and its c, s, tx, ty
 *    and tz are finite (the de-skew's usable clause without its c > 0: fx_track_landmarks's good link under require_flags).  Usable:
 *    the motion m is link b - 1, FX_FOLLOW_LINK, motion = b - 1.  Otherwise, if a link p in [f, b - 1) was usable: m is the latest
 *    such link, FX_FOLLOW_COASTED (constant velocity: the last usable motion applied again), motion = p.  Otherwise
 *    FX_FOLLOW_HELD.  With a motion the prior is the track's good-link composition p* o m, fp64, no contraction, no fma, no
 *    renormalisation: c = pc mc - ps ms, s = ps mc + pc ms, tx = (pc mtx - ps mty) + ptx, ty = (ps mtx + pc mty) + pty,
 *    tz = ptz + mtz; its segment is start_poses[j]'s and its flags are 0.  The prior is p* itself, all 48 bytes, with
 *    FX_FOLLOW_HELD alone and motion = 0xffffffff, when there is no motion and also when p* is not finite (c, s, tx, ty or tz),
 *    when any of the five composed values is not finite, or when b >= S (beyond the block's scans).  No NaN is ever produced and
 *    stored: the bit pattern of a default NaN differs between processors, and the contract is bit for bit.
 * 3. The fix: out[b] and the map_id_of_row / nearest_of_row words of scan b's rows are what fx_map_localize writes for scan b
 *    under that prior and opt.loc (the same device functions): b >= S gets FX_LOC_NO_SCAN, a prior that is not finite
 *    FX_LOC_BAD_PRIOR.
 * 4. streak = the number of consecutive scans of the chain, up to and including b, whose record lacks FX_LOC_VALID (0 behind a
 *    VALID scan).  FX_FOLLOW_LOST iff streak >= max_lost.  The chain goes on either way: the caller decides when to call
 *    fx_map_relocalize.
 * 5. poses[b] = out[b].pose when poses_device is given: a contiguous fx_pose array for a second round of fx_map_localize, for
 *    fx_map_loop_correct_poses or for the next batch.
 * All n_scans records of out, follow and poses are written and nothing behind them; all q_max_rows words of both row arrays are
 * written, -1 outside the scans' rows.
 * The start pose is read on the device, so no host read stands between two batches: a batch that overlaps the last by one scan
 * passes &out_prev[last].pose, a first batch &reloc[b].pose of fx_map_relocalize, a mapping run fx_map_get's last_pose address.
 * FX_ERR_INVALID_ARG with the reason in fx_last_error(), nothing launched, no output byte touched: fx_map_localize's own list
 * applied to opt.loc; a NULL start_poses_device, out_device or follow_device; a NULL links_device when some chain has more than one
 * scan; max_lost == 0; require_flags bits beyond the FX_REG_* flags; reserved != 0; records not 8-byte (words: 4-byte) aligned.
 * The same bytes from run to run and with any number of contexts in flight.  Limits: a chain is sequential by definition (one
 * workgroup walks it); the search distance does not widen with the streak, the motion model is constant velocity, and the call
 * never relocalises by itself.  New in 0.7 (added symbols only). */
typedef struct fx_follow_options {  /* 48 B */
  fx_localize_options loc;  /* fx_localize_options_default's, except segment = FX_LOC_ANY_SEGMENT */
  uint32_t chain_scans;     /* scans a chain; 0 (default): one chain of all n_scans */
  uint32_t require_flags;   /* FX_REG_* bits a link must carry to be usable; default FX_REG_VALID */
  uint32_t max_lost;        /* FX_FOLLOW_LOST from this many scans in a row without FX_LOC_VALID; >= 1, default 5 */
  uint32_t reserved;        /* 0 */
} fx_follow_options;
#define FX_FOLLOW_START 0x1u    /* the first scan of its chain: the prior is the start pose */
#define FX_FOLLOW_LINK 0x2u     /* the prior is the pose before composed with the scan's own link */
#define FX_FOLLOW_COASTED 0x4u  /* the link was unusable: the chain's last usable motion was applied again */
#define FX_FOLLOW_HELD 0x8u     /* the prior is the pose of the scan before, bit for bit */
#define FX_FOLLOW_LOST 0x10u    /* streak >= max_lost */
#define FX_FOLLOW_NO_MOTION 0xffffffffu
typedef struct fx_follow_scan {  /* 64 B, one per scan */
  fx_pose prior;                 /* the prior scan b was localised under */
  uint32_t flags, motion;        /* motion: index of the link applied, FX_FOLLOW_NO_MOTION: none */
  uint32_t streak, reserved;     /* scans in a row up to this one without FX_LOC_VALID; 0 */
} fx_follow_scan;
void fx_follow_options_default(fx_follow_options *o);
fx_status fx_map_follow(fx_ctx *ctx, fx_map *map,
    const void *kp_block_device, uint32_t max_scans, uint32_t max_total_keypoints,
    const fx_registration *links_device,        /* links[p], p < n_scans - 1: scan p + 1 -> scan p (pairs_consecutive) */
    const fx_pose *start_poses_device,           /* [n_chains], on the DEVICE */
    uint32_t n_scans, uint32_t q_max_rows, const fx_follow_options *opt /* NULL: defaults */,
    fx_localization *out_device /* [n_scans] */, fx_follow_scan *follow_device /* [n_scans] */,
    fx_pose *poses_device /* [n_scans] or NULL */,
    int32_t *map_id_of_row_device /* [q_max_rows] */, int32_t *nearest_of_row_device /* [q_max_rows] or NULL */);

/* Rotation matrix of rotateCloud (ref: node.cpp:161-164): R = Ry(pitch)*Rx(roll)
 * through Eigen's AngleAxisf -> Quaternionf -> toRotationMatrix, all float. Host only. */
void fx_rotation_from_roll_pitch(double roll, double pitch, float R[9]);
/* ShapeContext3DEstimation::initCompute tables (radii[16], theta[12], phi[13], lut[1980])
 * for descriptor_radius R: rmin = R/10 (ref: node.cpp:350-352). Host only. */
void fx_sc3d_tables(double R, float *radii16, float *theta12, float *phi13, float *lut1980);
/* x-axis of keypoint ordinal k from the boost::mt19937(12345) stream of 3DSC. Host only. */
void fx_sc3d_xaxis(uint32_t k, float xy[2]);

/* Synthetic scan generator (the reference ships no data).
 * Writes n_rings*n_az float4 (x,y,z,0) in firing order (azimuth-major, ring-minor). Host only. */
typedef struct fx_synth_cfg {
  uint32_t n_rings, n_az;
  double el0_deg, el_step_deg;
  uint32_t n_poles;
  double pole_radius, pole_height;
  double x_lo, x_hi, y_lo, y_hi; /* pole centres uniform in this box */
  double sensor_height;          /* ground plane z = -sensor_height */
  double wall_radius;            /* enclosing cylinder, always hit => fixed N */
  uint64_t seed;
} fx_synth_cfg;
void fx_synth_cfg_vlp16(fx_synth_cfg *c, uint64_t seed);
uint32_t fx_synth_scan(const fx_synth_cfg *c, float *xyzi_out, uint32_t capacity_points);

/* ---- test entry points: only in the TEST build of the library (lib/libfx_hip_test.so, compiled with -DFX_TEST_HOOKS,
 * which also reads the environment hooks tests use to push work through the rarely used tiers).  The product library
 * exports none of them and contains none of the k_test_* kernels. ---- */
#ifdef FX_TEST_HOOKS
/* Test hook: host build of the cluster-order replay the kernels run on one GPU lane
 * (csrc/fx_sort_replay.h).  perm_out[s] = ordinal of the cluster PCL returns at position s. */
void fx_test_sort_replay(const uint32_t *sizes, uint32_t n, uint32_t *perm_out);
/* same, with the final insertion phase replaced by the stable ranking the kernels use */
void fx_test_sort_replay_ranked(const uint32_t *sizes, uint32_t n, uint32_t *perm_out);
/* same, with the partition step stated through position lists (the rule the wavefront version follows) */
void fx_test_sort_replay_lists(const uint32_t *sizes, uint32_t n, uint32_t *perm_out);
/* Test hook: the replay as the kernels run it (wavefront partition phase + ranking) on device `device`,
 * one workgroup per sequence; n <= 192 per sequence.  sizes / perm_out: host arrays [n_seq][n]. */
fx_status fx_test_sort_replay_device(int device, const uint32_t *sizes, uint32_t n_seq, uint32_t n, uint32_t *perm_out);
/* Test hook: cc_order itself, the routine the ring and merge kernels call (acceptance by size, discovery ordinals, the dispatch
 * over the partition forms, the stable ranking), one workgroup of nt threads (64, 256 or 1024) per sequence.  Entry i of a
 * sequence is a component of its own of sizes[seq][i] (<= 65535) members; those with min_sz <= size <= max_sz are accepted.
 * gs = 0: croot / crec / tmp of ccap[seq] entries each in LDS; gs != 0: in a scratch region of HBM, the block helpers and the
 * sort stack in LDS, as the slow tier places them.  n, ccap[seq] <= 4096.
 * n_c_out[seq]: accepted entries.  If n_c_out[seq] <= ccap[seq]: perm_out[seq][s] = discovery ordinal (rank among the accepted,
 * in index order) of the cluster PCL returns at position s, root_out[seq][ordinal] = its index (root_out may be NULL), s and
 * ordinal < n_c_out[seq]; the rest of both rows, and all of them otherwise, is 0xffffffff.
 * guard_bad_out[seq]: how many of the guard words behind the three arrays the routine changed (0 whether it fits or not). */
fx_status fx_test_cc_order_device(int device, const uint32_t *sizes, uint32_t n_seq, uint32_t n, uint32_t min_sz, uint32_t max_sz,
                                  const uint32_t *ccap, uint32_t nt, int gs, uint32_t *perm_out, uint32_t *root_out, uint32_t *n_c_out,
                                  uint32_t *guard_bad_out);
/* Test hook: the two evaluations of a point's elevation angle the filter stage has (ref: node.cpp:147-156) on host
 * points xyz[n][3]: the table-driven one (fast_out, and whether it vouches for its value: fast_ok_out) and the one
 * through the library's fp64 atan2 that takes the points it does not vouch for (exact_out). */
fx_status fx_test_elevation_device(int device, const float *xyz, uint32_t n, float *fast_out, uint8_t *fast_ok_out, float *exact_out);
/* Test hook: 3DSC's local point density count as the descriptor kernels evaluate it (two points per packed instruction, the
 * comparison folded into a clamped fma) and as the plain `dist2 < r2` it replaces: for each of nq queries (xyzw records) the
 * number of the n support points (xyzw records) closer than sqrt(r2), both ways. */
fx_status fx_test_within_device(int device, const float *support_xyzw, uint32_t n, const float *query_xyzw, uint32_t nq, float r2,
                                uint32_t *packed_out, uint32_t *plain_out);
/* Test hook: what the support gather of the context's last batch left on the device, copied to the host.  Waits for the context's
 * stream, launches nothing and writes nothing on the device.  Nothing after the gather (k_gather*, k_rng_ord) writes what is copied
 * here — the descriptor tiers only load the lists, the overflow region, the counts, the row tables, the work lists and their
 * counters —, so what is read after a batch is what the gather left.
 * `info` is always filled: the constants a reference must not re-derive loosely, the sizes of the arrays, the work lists' counters.
 * `out` may be NULL (sizes only); any of its pointers may be NULL (not copied).  rows = info->rows below. */
typedef struct fx_test_gather_info {
  uint32_t batch;        /* scans of the last batch */
  uint32_t rows;         /* descriptor rows of the batch: min(kp_offset[batch], max_total_keypoints) */
  uint32_t near_words;   /* words of a scan's near-sector bits (bit s of the scan, points 4 s .. 4 s + 3: bit s % 32 of word s / 32) */
  uint32_t list_cap;     /* entries of a row's list */
  uint32_t ovf_cap;      /* entries of a scan's overflow region */
  uint32_t ovf_stored;   /* the largest min(ovf_cnt, ovf_cap) of the batch's scans: entries a scan copied to ovf_pts / ovf_kp */
  uint32_t dense_min;    /* list rows hold up to min(list_cap, dense_min) support points */
  uint32_t max_dense_rows;
  float r2_support, r2_search, box_margin;
  uint32_t n_list, n_wave, n_group[3], n_dense; /* the work lists' counters */
} fx_test_gather_info;
typedef struct fx_test_gather_out {
  uint32_t *near_bits;  /* [batch][near_words] */
  uint32_t *s_cnt;      /* [rows] */
  float *s_pts;         /* [rows][list_cap][4]: x, y, z rotated, the point's index as bits */
  uint32_t *ovf_cnt;    /* [batch] */
  float *ovf_pts;       /* [batch][ovf_stored][4] */
  uint32_t *ovf_kp;     /* [batch][ovf_stored] */
  uint32_t *row_map;    /* [rows][2]: scan, keypoint */
  float *row_kp;        /* [rows][4] */
  uint8_t *row_class;   /* [rows] */
  float *row_xa;        /* [rows][2] */
  uint32_t *list_desc;  /* [min(n_list, rows)] */
  uint32_t *wave_desc;  /* [min(n_wave, rows)] */
  uint32_t *group_desc; /* [3][rows]: the leading min(n_group[c], rows) of class c */
  uint32_t *dense_rows; /* [min(n_dense, max_dense_rows)] */
} fx_test_gather_out;
fx_status fx_test_gather_state(fx_ctx *ctx, fx_test_gather_info *info, const fx_test_gather_out *out);
#endif /* FX_TEST_HOOKS */

#ifdef __cplusplus
}
#endif
#endif /* FX_H_ */
