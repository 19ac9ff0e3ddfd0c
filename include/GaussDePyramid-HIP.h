// GaussDePyramid-HIP.h — drop-in MI355X replacement for the reference's pyramid classes.
//
// Usage is the reference's own (main.cpp:2-13, 61-74): swap the #include line and the class name,
//     #include "GaussDePyramid-HIP.h"
//     GaussPyramid_hip g(p, n, 2);
//     g.GenerateDoG();            // GaussFilter + DoG of every octave on the GPU
//     g.GaussPy[o][s][r][c] ...   // host float**** mirror, as in GuassDePyramid.h:16
// and link with -lgdp (libgdp.so, sift-parallel-optimization_amd/lib).  The class mirrors
// `class GaussPyramid` (GuassDePyramid.h:11-29) member for member; every method is a thin
// caller of the C ABI in gdp.h.  Host code only: this header needs no HIP headers and compiles
// with plain g++.
//
// Semantics kept from the reference:
//  - the constructor deep-copies img[0:len][0:len] and calls GaussPyInit() (:36-58);
//  - GaussPyInit() refills every level with the decimated input (:60-87);
//  - GaussFilter(o) window-multiplies every scale of octave o in place (:106-134);
//  - GenerateDoG() = GaussFilter + DoG per octave on the CURRENT contents (:136-149), so calling
//    it twice without GaussPyInit() filters twice, like the timing loop of main.cpp:66-73;
//  - GaussPy holds [layer][S+3][len_o][len_o] floats allocated with new[] (:63-72), freed by the
//    destructor (:151-170).
// GaussPy is two-way state, as in the reference, where the float**** IS the pyramid and every
// method works on whatever the caller left in it (:16, :122-131, :140-146):
//  - mirror_host = true (default): before each mutating call (GaussFilter, GenerateDoG,
//    GenerateDoG_mpi) the host GaussPy is uploaded to the device, and after it the device pyramid
//    is copied back into GaussPy; GaussPyInit re-reads `data` (:80).  A caller may write
//    g.GaussPy[o][s][r][c] (or g.data[r][c]) at any time and the next call processes the edit.
//    Cost: the upload is only of what the caller wrote.  The mirror (gdp_host_alloc_tracked: the
//    pages GaussPy points into, DMA'd through a second, registered mapping of the same memory) is
//    write-protected whenever it equals the device copy (gdp_host_arm); a CPU write to a page
//    faults once and is recorded, and the next mutating call uploads only the written pages
//    (gdp_upload_image_written, gdp_generate_dog_mirrored_written) — none in main.cpp's loop
//    (:66-73), which never writes GaussPy.  The D2H copy back is one per call (447 MB at 4096^2,
//    INTEGRATION §2c); GenerateDoG / GenerateDoG_mpi overlap it with the kernel over row chunks
//    (best-effort: the copy streams share the process's hardware queues — 4 on the MI355X boxes —
//    with every other stream and context, so under concurrent work they may serialise; the result
//    is the same either way).
//    Writes that do not fault on the CPU (read(2) into GaussPy — EFAULT on a protected page —, or
//    DMA into it) are not seen: call TrackWrites(false) first, and every call uploads the whole
//    mirror as before (also the fallback when page protection is unavailable).
//    DeferDownload(true) (opt-in; or GDP_DEFER_DOWNLOAD=1 in the environment): the copy back is deferred too — after a mutating call GaussPy's
//    pages are inaccessible and the first access to one fetches its neighbourhood from the device
//    (gdp_host_defer); main.cpp's loop then moves nothing over PCIe.  Reads see the same values.
//  - mirror_host = false: the device pyramid is the state; GaussPy is refreshed only by
//    SyncHost(), and host edits reach the device only through SyncDevice() — or set
//    `host_dirty = true` after editing and the next mutating call uploads first (then clears it).
// Row pointers the caller re-seated (GaussPy[o][s][r] = other array) are honoured both ways: the
// single raw DMA copy is used only while every row still points into the pinned mirror.
// Errors: the reference never reports them; a failing libgdp call here prints gdp_last_error()
// and aborts rather than continuing on bad state.
#ifndef SIFT_GAUSSDEPYRAMID_HIP_H
#define SIFT_GAUSSDEPYRAMID_HIP_H

// What a caller of the replaced header gets transitively: GaussDePyramid-MPI.h:8-13 pulls in
// <iostream>, <chrono>, <math.h> and <sys/time.h>, and main.cpp:62-69 relies on <chrono>.
#include <math.h>
#include <sys/time.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "gdp.h"

class GaussPyramid_hip {
public:
    int** data;  // copy of the input image (:13)
    GaussPyramid_hip();
    GaussPyramid_hip(int** img, int len, int S, int device = 0);
    float**** GaussPy;  // [layer][S+3][len_o][len_o] host mirror (:16)
    void GaussPyInit();
    void output();
    void GaussFilter(int theLayer);
    void GenerateDoG();
    // GaussPyramid_mpi::GenerateDoG_mpi (GaussDePyramid-MPI.h:265-335), the call main.cpp:68 makes.
    // The reference fans scales out over >= S+4 MPI ranks and collects on rank S+3; here one GPU
    // does the whole pyramid and GaussPy ends as that collector's GaussPy.  Like the method it
    // replaces, it centres every window on the INTEGER octave length (`l = float(len - 1) / 2.0`,
    // :273 — GDP_CENTRE_INTLEN), not on the float-halved length GaussFilter/GenerateDoG use
    // (:133-183, GuassDePyramid.h:107-115); the two differ when n is not a multiple of
    // 2^(layer-1) (n = 100, 1000, ...).  The context returns to the serial centre afterwards, so
    // GaussFilter/GenerateDoG keep theirs.  Unlike the reference (MPI_Init/MPI_Finalize inside)
    // it may be called any number of times; each call continues from the current contents.
    void GenerateDoG_mpi(int argc, char** argv);
    void GenerateDoG_mgpu(int argc, char** argv) { GenerateDoG_mpi(argc, argv); }  // SURVEY §8(f2) name
    // Extension (no reference counterpart): the strict scale-space extrema of the current pyramid
    // (levels 0..S+1 as DoG levels), found on the device and returned sorted by (octave, scale, row,
    // col) — gdp_detect_extrema in gdp.h has the exact rules.  Pending host edits of GaussPy are
    // uploaded first, as before every mutating call; the pyramid itself is not changed, so GaussPy
    // is neither published nor downloaded again.  At most the context's keypoint capacity (65536
    // unless gdp_set_keypoint_capacity(context(), n) raised it) records come back.
    std::vector<gdp_keypoint> DetectExtrema(float contrast_threshold = 0.f, float edge_ratio = 0.f);
    // Extension: the keypoints of the last DetectExtrema localised to sub-sample precision on the
    // device (gdp_refine_keypoints in gdp.h has the exact rule: quadratic fit, at most 5 moves,
    // |interp| > contrast, the edge test when edge_ratio != 0), sorted like gdp_download_refined.
    // Pending host edits of GaussPy are uploaded first; the pyramid itself is not changed.
    std::vector<gdp_keypoint_refined> RefineKeypoints(float contrast = 0.f, float edge_ratio = 0.f);
    // Extension: orientations of the last RefineKeypoints' records, assigned on the device
    // (gdp_orient_keypoints in gdp.h has the exact rule: the Gaussian level rebuilt from levels
    // s..S+2, a 36-bin gradient histogram, one record per peak within 80 % of the highest), sorted
    // like gdp_download_oriented.  Pending host edits of GaussPy are uploaded first; the pyramid
    // itself is not changed.  At most twice the keypoint capacity records come back.
    std::vector<gdp_keypoint_oriented> OrientKeypoints();
    // Extension: the 128-byte SIFT descriptors of the last OrientKeypoints' records, computed on the
    // device (gdp_describe_keypoints in gdp.h has the exact rule: the Gaussian level rebuilt from
    // levels s..S+2, a 4 x 4 x 8 gradient histogram rotated to the keypoint's angle, normalised,
    // clipped and quantised), sorted like gdp_download_described: one record per oriented record.
    // Pending host edits of GaussPy are uploaded first; the pyramid itself is not changed.
    std::vector<gdp_keypoint_described> DescribeKeypoints();
    // Extension: match the last DescribeKeypoints' records of this pyramid (the queries) against
    // those of `other` (the train side; it may be *this; same device) on the device
    // (gdp_match_descriptors in gdp.h has the exact rule: exact squared L2 distances on the i8 matrix
    // cores, nearest and second nearest with ties to the lowest index, Lowe's ratio test with `ratio`
    // (0: off), a distance cap and the mutual test), sorted by `query` like gdp_download_matches.
    // Indices name the lists in device order; qx, qy, tx, ty are the keypoints' image coordinates.
    // Neither pyramid nor any list is changed; the match object lives for the call only.
    std::vector<gdp_match_record> MatchDescriptors(GaussPyramid_hip& other, float ratio = 0.8f,
                                                   uint32_t max_distance = 0xffffffffu, bool mutual = false);
    // Extension: the homography that most of `matches` (MatchDescriptors' records, in the order given)
    // agree on, by RANSAC on the device (gdp_fit_homography in gdp.h has the exact rule: `hypotheses`
    // four-point fits in float64 without a division, each scored in float32 against every match with
    // the transfer error `threshold` in pixels; the largest count wins, ties to the lowest index).
    // Returns the model record: h[] maps (qx, qy, 1) to (tx, ty, 1) up to scale; hypothesis ==
    // 0xffffffff when fewer than max(min_inliers, 4) matches agree.  *inliers (when not NULL) gets
    // the matches the model accepts, sorted by `query`.  The list is the caller's, so the result is
    // a function of the arguments alone.  Nothing of the pyramid or its lists is changed; the fit
    // object lives for the call only.
    gdp_homography FitHomography(const std::vector<gdp_match_record>& matches, std::vector<gdp_match_record>* inliers = nullptr,
                                 uint32_t hypotheses = 1024, uint32_t seed = 0, float threshold = 3.0f, uint32_t min_inliers = 4);
    // Extension: FitHomography followed, on the same fit object and stream with no host read in between,
    // by `rounds` (1..8) rounds of the least-squares refit of the model over its inliers
    // (gdp_refit_homography in gdp.h has the exact rule: exact 128-bit integer moments of the inlier
    // coordinates quantised to 1/256 px, one 8 x 8 solve in float64; a round's candidate replaces the
    // model and the inliers when it accepts at least as many matches under `refit_threshold`).  Returns
    // the model record after the refit; *inliers as for FitHomography, *record (when not NULL) the
    // refit record.  hypothesis and sample[] stay the RANSAC winner's.
    gdp_homography RefitHomography(const std::vector<gdp_match_record>& matches, std::vector<gdp_match_record>* inliers = nullptr,
                                   gdp_refit_record* record = nullptr, uint32_t rounds = 1, float refit_threshold = 3.0f,
                                   uint32_t hypotheses = 1024, uint32_t seed = 0, float threshold = 3.0f, uint32_t min_inliers = 4);
    // Extension: `other`'s input image resampled into this pyramid's frame (GDP_WARP_TRAIN_TO_QUERY), or
    // this pyramid's into `other`'s (GDP_WARP_QUERY_TO_TRAIN, under the normalised adjugate), on the
    // device (gdp_warp_image in gdp.h has the exact rule: `h` maps this pyramid's (x, y) to `other`'s,
    // as FitHomography's h[] does; bilinear, ties to even, uncovered pixels store `fill`).  Returns the
    // image row-major in *rows x *cols (either may be NULL) and, in *record when not NULL, the matrix
    // used, `covered` and `sad`, the sum of absolute differences to the destination frame's image over
    // the covered pixels.  Nothing of either pyramid or its lists is changed; the warp object lives for
    // the call only.
    std::vector<int32_t> WarpImage(GaussPyramid_hip& other, const float h[9], int direction = GDP_WARP_TRAIN_TO_QUERY,
                                   int32_t fill = 0, gdp_warp_record* record = nullptr, int* rows = nullptr, int* cols = nullptr);
    // Extension: the last DescribeKeypoints' records of this pyramid matched against those of `other`
    // again, each query only against the records within `radius` pixels (in x and in y) of its
    // projection under `h`, on the device (gdp_match_guided in gdp.h has the exact rule: `h` maps this
    // pyramid's (x, y) to `other`'s, as FitHomography's h[] does; exact nearest and second nearest among
    // the candidates, the ratio test (0: off) and the cap of MatchDescriptors; `unique` keeps one query
    // per train record), sorted by `query`.  Neither pyramid nor any list is changed; the object lives
    // for the call only.
    std::vector<gdp_match_record> GuidedMatch(GaussPyramid_hip& other, const float h[9], float radius = 3.0f, float ratio = 0.0f,
                                              uint32_t max_distance = 0xffffffffu, bool unique = true);
    ~GaussPyramid_hip();
    bool initialized;
    bool mirror_host;  // GaussPy two-way: upload before / download after every mutating call (default true)
    bool host_dirty;   // mirror_host == false: the caller edited GaussPy / data; the next call uploads first
    void SyncHost();   // copy the device pyramid into GaussPy now
    void SyncDevice(); // copy GaussPy (the host pyramid, possibly edited) into the device pyramid now
    // Write tracking of the mirror (default on when pinned memory and page protection are
    // available): off, every mutating call uploads the whole mirror (see the header comment).
    void TrackWrites(bool on);
    bool tracking_writes() const { return track_; }
    // Bytes of GaussPy in pages written since the mirror was last armed (the next call's upload),
    // or -1 when no such record exists (not tracked / not armed: the next call uploads everything).
    long long written_bytes() const {
        size_t b = 0;
        return track_ && armed_ && gdp_host_written_bytes(host_, &b) == GDP_OK ? (long long)b : -1;
    }
    // Deferred download (opt-in, needs the write-tracked mirror): with mirror_host, a mutating call
    // leaves GaussPy's pages inaccessible instead of copying the device pyramid back, and the first
    // access to one has its neighbourhood fetched (gdp_host_defer).  A caller that does not read
    // GaussPy between calls — main.cpp's timing loop (:66-73) — moves nothing over PCIe; one that
    // reads it gets the same values as with the eager copy.  Off (the default), or for a caller
    // that hands GaussPy to system calls (write(2) of a deferred page fails with EFAULT) or straight
    // to HIP copies: call SyncHost() / DeferDownload(false) before those.  Returns whether it is on.
    bool DeferDownload(bool on);
    bool deferring() const { return defer_; }
    // Bytes of GaussPy still to be fetched (inaccessible pages), or -1 when not deferring.
    long long stale_bytes() const {
        size_t b = 0;
        return defer_ && gdp_host_deferred_stats(host_, &b, nullptr, nullptr) == GDP_OK ? (long long)b : -1;
    }
    gdp_ctx* context() const { return ctx_; }

protected:
    int length;
    int S;
    int layer;
    float* filter;  // unused (taps live on the device); kept for layout parity with :28
    gdp_ctx* ctx_;
    bool fresh_;  // contents == GaussPyInit(): GenerateDoG may use the fused build kernel
    float* host_; // pinned host pyramid in the device layout that the GaussPy rows point into
                  // (gdp_host_alloc); NULL: rows are separate new[] arrays (pinned memory refused)
    bool track_;  // host_ is write-tracked (gdp_host_track)
    bool armed_;  // the device pyramid equals host_ as of its last arming and the pages written
                  // since are recorded: the next mutating call may upload only those
    bool defer_;  // DeferDownload: mutating calls end in gdp_host_defer instead of SyncHost
    gdp_orient* orient_ = nullptr;  // OrientKeypoints' state, created on its first call, destroyed before ctx_
    gdp_describe* describe_ = nullptr;  // DescribeKeypoints' state, created on its first call, destroyed before orient_
    // rows_in_mirror_() is a walk over every row pointer (41k at 4096^2, tens of microseconds):
    // each public call takes it once (CallScope) and its helpers reuse the answer — the caller
    // cannot re-seat a row while one of its calls runs
    mutable int rows_memo_ = -1;
    mutable int call_depth_ = 0;
    struct CallScope {
        const GaussPyramid_hip* g;
        explicit CallScope(const GaussPyramid_hip* g_) : g(g_) {
            if (g->call_depth_++ == 0) g->rows_memo_ = g->rows_scan_() ? 1 : 0;
        }
        ~CallScope() {
            if (--g->call_depth_ == 0) g->rows_memo_ = -1;
        }
    };
    bool rows_in_mirror_() const { return rows_memo_ >= 0 ? rows_memo_ != 0 : rows_scan_(); }
    bool rows_scan_() const {  // every GaussPy row still where the constructor put it
        if (!host_) return false;
        for (int o = 0; o < layer; ++o)
            for (int s = 0; s < S + 3; ++s) {
                const float* lev = host_ + gdp_level_offset(ctx_, 0, o, s);
                const int n = length >> o;
                for (int r = 0; r < n; ++r)
                    if (GaussPy[o][s][r] != lev + (size_t)r * n) return false;
            }
        return true;
    }
    void keep_deferred_() {  // before a mutating call: a deferred GaussPy that the call will not
        // defer again (mirror_host off, rows re-seated) is fetched now, while the device still
        // holds what it shows
        if (defer_ && !(mirror_host && rows_in_mirror_())) check_(ctx_, gdp_host_fetch(host_), "DeferDownload");
    }
    void pull_host_() {  // before a mutating call: the caller's GaussPy is the state
        keep_deferred_();
        const bool clean = armed_;
        armed_ = false;  // the call changes the device; SyncHost re-arms
        if (!(mirror_host || host_dirty)) return;
        if (clean && rows_in_mirror_())
            check_(ctx_, gdp_upload_image_written(ctx_, 0, host_), "SyncDevice");
        else
            upload_();
        host_dirty = false;
        fresh_ = false;  // the contents are the caller's now, not necessarily GaussPyInit's
    }
    void upload_() {  // the whole mirror: one H2D DMA copy, or staged row gathers
        check_(ctx_, rows_in_mirror_() ? gdp_upload_image_raw(ctx_, 0, host_)
                                       : gdp_upload_pyramid_rows(ctx_, 0, (const float* const* const* const*)GaussPy),
               "SyncDevice");
    }
    void arm_() {  // host_ == the device copy now: protect it again (or stop tracking if refused)
        armed_ = false;
        if (!track_ || !rows_in_mirror_()) return;
        if (gdp_host_arm(host_) == GDP_OK) {
            armed_ = true;
        } else {
            (void)gdp_host_untrack(host_);
            track_ = false;
        }
    }
    int mirrored_call_() {  // gdp_generate_dog_mirrored(_written) on host_, the status returned
        const bool clean = armed_;
        armed_ = false;
        return clean ? gdp_generate_dog_mirrored_written(ctx_, 0, host_) : gdp_generate_dog_mirrored(ctx_, 0, host_);
    }
    void mirrored_done_() {  // after a successful mirrored call: host_ == the device copy
        host_dirty = false;
        fresh_ = false;
        arm_();
    }
    void mirrored_(const char* what) {
        check_(ctx_, mirrored_call_(), what);
        mirrored_done_();
    }
    bool piped_() const { return mirror_host && !defer_ && rows_in_mirror_(); }  // the mirrored single call
    void publish_() {  // after a mutating call with mirror_host: GaussPy shows the device pyramid
        if (defer_ && rows_in_mirror_() && gdp_host_defer(ctx_, 0, host_) == GDP_OK) {
            armed_ = true;  // pages fetched and then written are recorded from here on
            return;
        }
        SyncHost();
    }
    static void check_(gdp_ctx* c, int status, const char* what) {
        if (status != GDP_OK) fail_(what, gdp_last_error(c), status);
    }
    // every failure ends here, with the last-error text of the object the call was made on
    [[noreturn]] static void fail_(const char* what, const char* last, int status) {
        std::fprintf(stderr, "GaussPyramid_hip::%s failed: %s (%s)\n", what, gdp_status_string(status), last);
        std::abort();
    }
    // a stage object's call: its text is asked for after the call, from `h` (NULL for a failed create)
    template <class H>
    static void check_(const char* what, const char* last_error(const H*), const H* h, int status) {
        if (status != GDP_OK) fail_(what, last_error(h), status);
    }
    void ensure_described_(const char* what) {  // a pyramid that was never described has an empty list
        if (!orient_) check_<gdp_orient>(what, gdp_orient_last_error, nullptr, gdp_orient_create(&orient_, ctx_, 0));
        if (!describe_)
            check_<gdp_describe>(what, gdp_describe_last_error, nullptr, gdp_describe_create(&describe_, ctx_, orient_, 0));
    }
    // count, size the vector, download, resize to what was stored; `lead` is the image of a per-image list
    template <class Rec, class H, class Count, class Download, class... Lead>
    static std::vector<Rec> list_(const char* what, const char* last_error(const H*), H* h, Count count, Download download,
                                  Lead... lead) {
        size_t found = 0, stored = 0;
        check_(what, last_error, h, count(h, lead..., &found));
        std::vector<Rec> out(found);
        check_(what, last_error, h, download(h, lead..., out.data(), out.size(), &stored, nullptr));
        out.resize(stored);
        return out;
    }
    // FitHomography and RefitHomography: one fit object for the call, `rounds` = 0 without the refit
    gdp_homography fit_(const char* what, const std::vector<gdp_match_record>& matches, std::vector<gdp_match_record>* inliers,
                        uint32_t hypotheses, uint32_t seed, float threshold, uint32_t min_inliers, uint32_t rounds, float refit_threshold,
                        gdp_refit_record* record);
    static int download_refined_(gdp_ctx* c, int b, gdp_keypoint_refined* host, size_t capacity, size_t* stored, size_t*) {
        return gdp_download_refined(c, b, host, capacity, stored);  // the one list without a `found` output
    }
};

inline GaussPyramid_hip::GaussPyramid_hip()
    : data(nullptr), GaussPy(nullptr), initialized(false), mirror_host(true), host_dirty(false), length(0), S(0),
      layer(0), filter(nullptr), ctx_(nullptr), fresh_(false), host_(nullptr), track_(false), armed_(false),
      defer_(false) {}

inline GaussPyramid_hip::GaussPyramid_hip(int** img, int len, int S_, int device)
    : data(nullptr), GaussPy(nullptr), initialized(false), mirror_host(true), host_dirty(false), length(len), S(S_),
      layer(0), filter(nullptr), ctx_(nullptr), fresh_(false), host_(nullptr), track_(false), armed_(false),
      defer_(false) {
    data = new int*[len];
    for (int i = 0; i < len; ++i) {
        data[i] = new int[len];
        for (int j = 0; j < len; ++j) data[i][j] = img[i][j];
    }
    layer = gdp_octaves_for(len);  // :48-53
    filter = new float[len];
    check_(nullptr, gdp_create(&ctx_, len, len, S, layer, 1, device), "GaussPyramid_hip");
    check_(ctx_, gdp_set_input_rows(ctx_, 0, (const int32_t* const*)data, nullptr), "GaussPyramid_hip");
    // The GaussPy rows (:16, one new float[] per row in the reference) point into ONE pinned host
    // buffer laid out like the device pyramid, so SyncHost is a single DMA copy at the full PCIe
    // rate; if pinned memory is refused, separate rows and the staged scatter are used instead.
    void* h = nullptr;
    // Write-tracked when the platform allows it (gdp_host_alloc_tracked: a registered DMA view and a
    // protectable CPU view of the same pages), else plain pinned memory and whole uploads.
    const size_t mirror_bytes = gdp_image_floats(ctx_) * sizeof(float);
    if (gdp_host_alloc_tracked(mirror_bytes, &h) == GDP_OK) {
        host_ = static_cast<float*>(h);
        track_ = true;
    } else if (gdp_host_alloc(mirror_bytes, &h) == GDP_OK) {
        host_ = static_cast<float*>(h);
    }
    GaussPy = new float***[layer];
    for (int o = 0; o < layer; ++o) {
        const int n = len >> o;
        GaussPy[o] = new float**[S + 3];
        for (int s = 0; s < S + 3; ++s) {
            GaussPy[o][s] = new float*[n];
            float* lev = host_ ? host_ + gdp_level_offset(ctx_, 0, o, s) : nullptr;
            for (int r = 0; r < n; ++r) GaussPy[o][s][r] = lev ? lev + (size_t)r * n : new float[n];
        }
    }
    check_(ctx_, gdp_init(ctx_, nullptr), "GaussPyramid_hip");  // GaussPyInit (:57); `data` just uploaded
    initialized = true;
    fresh_ = true;
    if (mirror_host) SyncHost();
    // GDP_DEFER_DOWNLOAD=1 in the environment turns the deferred download on for an unmodified
    // caller (main.cpp after the two-line switch)
    if (const char* e = std::getenv("GDP_DEFER_DOWNLOAD"))
        if (e[0] == '1') DeferDownload(true);
}

inline void GaussPyramid_hip::SyncHost() {  // one DMA copy (pinned mirror) or one staged copy per 64 MiB
    CallScope scope(this);
    check_(ctx_, rows_in_mirror_() ? gdp_download_image_raw(ctx_, 0, host_) : gdp_download_pyramid_rows(ctx_, 0, GaussPy),
           "SyncHost");
    arm_();
}

inline void GaussPyramid_hip::SyncDevice() {  // the inverse: the whole mirror, one H2D DMA copy or staged row gathers
    CallScope scope(this);
    upload_();
    host_dirty = false;
    fresh_ = false;  // the contents are the caller's now, not necessarily GaussPyInit's
    arm_();
}

inline void GaussPyramid_hip::TrackWrites(bool on) {
    CallScope scope(this);
    if (!on && track_) {
        check_(ctx_, gdp_host_untrack(host_), "TrackWrites");  // fetched if deferred; every page writable again
        track_ = armed_ = defer_ = false;
    } else if (on && !track_ && host_) {
        // armed by the next SyncHost (every mutating call with mirror_host ends in one)
        track_ = gdp_host_track(host_, gdp_image_floats(ctx_) * sizeof(float)) == GDP_OK;
    }
}

inline bool GaussPyramid_hip::DeferDownload(bool on) {
    CallScope scope(this);
    if (!on && defer_) check_(ctx_, gdp_host_fetch(host_), "DeferDownload");  // GaussPy complete again
    defer_ = on && track_ && host_;  // takes effect from the next mutating call
    return defer_;
}

inline void GaussPyramid_hip::GaussPyInit() {  // :60-87, from the CURRENT `data` (:80)
    CallScope scope(this);
    keep_deferred_();
    armed_ = false;  // every level is refilled on the device
    if (mirror_host || host_dirty)
        check_(ctx_, gdp_set_input_rows(ctx_, 0, (const int32_t* const*)data, nullptr), "GaussPyInit");
    host_dirty = false;  // every level is refilled: host edits of GaussPy are overwritten, as in :76-86
    check_(ctx_, gdp_init(ctx_, nullptr), "GaussPyInit");
    initialized = true;
    fresh_ = true;
    if (mirror_host) publish_();
}

inline void GaussPyramid_hip::GaussFilter(int theLayer) {
    CallScope scope(this);
    pull_host_();
    check_(ctx_, gdp_gauss_octave(ctx_, theLayer, nullptr), "GaussFilter");
    fresh_ = false;
    if (mirror_host) publish_();
}

inline void GaussPyramid_hip::GenerateDoG() {
    CallScope scope(this);
    if (piped_()) {
        // GaussPy mirrored in the pinned device-layout buffer: upload (only the pages written since
        // the last call when tracked), in-place pass and download in one call, pipelined over row
        // chunks
        mirrored_("GenerateDoG");
        return;
    }
    // on freshly initialised contents the fused single-pass build is bit-identical to
    // GaussFilter + DoG in place; otherwise run the in-place pass on what is there
    pull_host_();
    check_(ctx_, fresh_ ? gdp_build(ctx_, nullptr) : gdp_generate_dog(ctx_, nullptr), "GenerateDoG");
    fresh_ = false;
    check_(ctx_, gdp_sync(ctx_), "GenerateDoG");
    if (mirror_host) publish_();
}

inline void GaussPyramid_hip::GenerateDoG_mpi(int, char**) {
    CallScope scope(this);
    // switching centres selects the other device tap table (no drain, no re-upload after the
    // first call); both calls below are ordered on the context's stream
    const bool piped = piped_();  // see GenerateDoG
    if (!piped) pull_host_();
    check_(ctx_, gdp_set_window_centre(ctx_, GDP_CENTRE_INTLEN), "GenerateDoG_mpi");
    if (piped) {
        const int rc = mirrored_call_();
        check_(ctx_, gdp_set_window_centre(ctx_, GDP_CENTRE_SERIAL), "GenerateDoG_mpi");
        check_(ctx_, rc, "GenerateDoG_mpi");
        mirrored_done_();
        return;
    }
    const int rc = fresh_ ? gdp_build(ctx_, nullptr) : gdp_generate_dog(ctx_, nullptr);
    check_(ctx_, gdp_set_window_centre(ctx_, GDP_CENTRE_SERIAL), "GenerateDoG_mpi");
    check_(ctx_, rc, "GenerateDoG_mpi");
    fresh_ = false;
    check_(ctx_, gdp_sync(ctx_), "GenerateDoG_mpi");
    if (mirror_host) publish_();
}

inline std::vector<gdp_keypoint> GaussPyramid_hip::DetectExtrema(float contrast_threshold, float edge_ratio) {
    CallScope scope(this);
    const bool clean = armed_;
    pull_host_();
    armed_ = clean;  // the detection leaves the device pyramid alone: the record of written pages stays valid
    check_(ctx_, gdp_detect_extrema(ctx_, contrast_threshold, edge_ratio, nullptr), "DetectExtrema");
    return list_<gdp_keypoint>("DetectExtrema", gdp_last_error, ctx_, gdp_keypoint_count, gdp_download_keypoints, 0);
}

inline std::vector<gdp_keypoint_refined> GaussPyramid_hip::RefineKeypoints(float contrast, float edge_ratio) {
    CallScope scope(this);
    const bool clean = armed_;
    pull_host_();
    armed_ = clean;  // the refinement leaves the device pyramid alone, like the detection
    check_(ctx_, gdp_refine_keypoints(ctx_, contrast, edge_ratio, nullptr), "RefineKeypoints");
    return list_<gdp_keypoint_refined>("RefineKeypoints", gdp_last_error, ctx_, gdp_refined_count, download_refined_, 0);
}

inline std::vector<gdp_keypoint_oriented> GaussPyramid_hip::OrientKeypoints() {
    const char* const what = "OrientKeypoints";
    CallScope scope(this);
    const bool clean = armed_;
    pull_host_();
    armed_ = clean;  // the orientation leaves the device pyramid alone, like the detection
    if (!orient_) check_<gdp_orient>(what, gdp_orient_last_error, nullptr, gdp_orient_create(&orient_, ctx_, 0));
    check_(what, gdp_orient_last_error, orient_, gdp_orient_keypoints(orient_, nullptr));
    return list_<gdp_keypoint_oriented>(what, gdp_orient_last_error, orient_, gdp_oriented_count, gdp_download_oriented, 0);
}

inline std::vector<gdp_keypoint_described> GaussPyramid_hip::DescribeKeypoints() {
    const char* const what = "DescribeKeypoints";
    CallScope scope(this);
    const bool clean = armed_;
    pull_host_();
    armed_ = clean;  // the description leaves the device pyramid alone, like the detection
    ensure_described_(what);
    check_(what, gdp_describe_last_error, describe_, gdp_describe_keypoints(describe_, nullptr));
    return list_<gdp_keypoint_described>(what, gdp_describe_last_error, describe_, gdp_described_count, gdp_download_described, 0);
}

inline std::vector<gdp_match_record> GaussPyramid_hip::MatchDescriptors(GaussPyramid_hip& other, float ratio, uint32_t max_distance,
                                                                        bool mutual) {
    const char* const what = "MatchDescriptors";
    ensure_described_(what);
    other.ensure_described_(what);
    gdp_match* m = nullptr;
    check_<gdp_match>(what, gdp_match_last_error, nullptr, gdp_match_create(&m, describe_, other.describe_, 0, 0));
    // DescribeKeypoints ends in a blocking download, so nothing of `other` is still in flight on its stream
    check_(what, gdp_match_last_error, m, gdp_match_descriptors(m, 0, 0, ratio, max_distance, mutual ? 1 : 0, nullptr));
    std::vector<gdp_match_record> out = list_<gdp_match_record>(what, gdp_match_last_error, m, gdp_match_count, gdp_download_matches);
    gdp_match_destroy(m);
    return out;
}

inline gdp_homography GaussPyramid_hip::FitHomography(const std::vector<gdp_match_record>& matches, std::vector<gdp_match_record>* inliers,
                                                      uint32_t hypotheses, uint32_t seed, float threshold, uint32_t min_inliers) {
    return fit_("FitHomography", matches, inliers, hypotheses, seed, threshold, min_inliers, 0, 0.0f, nullptr);
}

inline gdp_homography GaussPyramid_hip::RefitHomography(const std::vector<gdp_match_record>& matches, std::vector<gdp_match_record>* inliers,
                                                        gdp_refit_record* record, uint32_t rounds, float refit_threshold,
                                                        uint32_t hypotheses, uint32_t seed, float threshold, uint32_t min_inliers) {
    if (rounds == 0) fail_("RefitHomography", "rounds must be in 1..8", GDP_ERR_ARG);
    return fit_("RefitHomography", matches, inliers, hypotheses, seed, threshold, min_inliers, rounds, refit_threshold, record);
}

inline gdp_homography GaussPyramid_hip::fit_(const char* what, const std::vector<gdp_match_record>& matches,
                                             std::vector<gdp_match_record>* inliers, uint32_t hypotheses, uint32_t seed, float threshold,
                                             uint32_t min_inliers, uint32_t rounds, float refit_threshold, gdp_refit_record* record) {
    ensure_described_(what);
    const size_t n = matches.size(), cap = n ? n : 1;
    gdp_match* m = nullptr;  // the fit object is made from a match object; its own list is never read here
    check_<gdp_match>(what, gdp_match_last_error, nullptr, gdp_match_create(&m, describe_, describe_, cap, 1));
    gdp_ransac* r = nullptr;
    check_<gdp_ransac>(what, gdp_ransac_last_error, nullptr, gdp_ransac_create(&r, m, cap, hypotheses));
    const gdp_match_record none{};
    check_(what, gdp_ransac_last_error, r, gdp_ransac_set_input(r, n ? matches.data() : &none, n));
    check_(what, gdp_ransac_last_error, r, gdp_fit_homography(r, hypotheses, seed, threshold, min_inliers, nullptr));
    if (rounds) check_(what, gdp_ransac_last_error, r, gdp_refit_homography(r, rounds, refit_threshold, nullptr));
    gdp_homography model;
    check_(what, gdp_ransac_last_error, r, gdp_download_homography(r, &model));
    if (record) check_(what, gdp_ransac_last_error, r, gdp_download_refit(r, record));
    if (inliers) *inliers = list_<gdp_match_record>(what, gdp_ransac_last_error, r, gdp_ransac_count, gdp_download_inliers);
    gdp_ransac_destroy(r);
    gdp_match_destroy(m);
    return model;
}

inline std::vector<int32_t> GaussPyramid_hip::WarpImage(GaussPyramid_hip& other, const float h[9], int direction, int32_t fill,
                                                        gdp_warp_record* record, int* rows, int* cols) {
    const char* const what = "WarpImage";
    ensure_described_(what);
    other.ensure_described_(what);
    gdp_match* m = nullptr;  // the warp object reaches the two contexts through a fit and a match object; no list is read
    check_<gdp_match>(what, gdp_match_last_error, nullptr, gdp_match_create(&m, describe_, other.describe_, 1, 1));
    gdp_ransac* r = nullptr;
    check_<gdp_ransac>(what, gdp_ransac_last_error, nullptr, gdp_ransac_create(&r, m, 1, 1));
    gdp_warp* w = nullptr;
    check_<gdp_warp>(what, gdp_warp_last_error, nullptr, gdp_warp_create(&w, r));
    check_(what, gdp_warp_last_error, w, gdp_warp_set_model(w, h));
    check_(what, gdp_warp_last_error, w, gdp_warp_image(w, direction, 0, 0, fill, nullptr));
    int height = 0, width = 0;
    check_(what, gdp_warp_last_error, w, gdp_device_warped(w, nullptr, nullptr, &height, &width, nullptr, nullptr));
    std::vector<int32_t> out((size_t)height * (size_t)width);
    check_(what, gdp_warp_last_error, w, gdp_download_warped(w, out.data(), (size_t)width));
    if (record) check_(what, gdp_warp_last_error, w, gdp_download_warp_record(w, record));
    if (rows) *rows = height;
    if (cols) *cols = width;
    gdp_warp_destroy(w);
    gdp_ransac_destroy(r);
    gdp_match_destroy(m);
    return out;
}

inline std::vector<gdp_match_record> GaussPyramid_hip::GuidedMatch(GaussPyramid_hip& other, const float h[9], float radius, float ratio,
                                                                   uint32_t max_distance, bool unique) {
    const char* const what = "GuidedMatch";
    ensure_described_(what);
    other.ensure_described_(what);
    gdp_match* m = nullptr;  // the two lists are the match object's sides; the fit object only carries the way to them
    check_<gdp_match>(what, gdp_match_last_error, nullptr, gdp_match_create(&m, describe_, other.describe_, 0, 0));
    gdp_ransac* r = nullptr;
    check_<gdp_ransac>(what, gdp_ransac_last_error, nullptr, gdp_ransac_create(&r, m, 1, 1));
    gdp_guided* g = nullptr;
    check_<gdp_guided>(what, gdp_guided_last_error, nullptr, gdp_guided_create(&g, r, 0));
    check_(what, gdp_guided_last_error, g, gdp_guided_set_model(g, h));
    check_(what, gdp_guided_last_error, g, gdp_match_guided(g, 0, 0, radius, ratio, max_distance, unique ? 1 : 0, nullptr));
    std::vector<gdp_match_record> out = list_<gdp_match_record>(what, gdp_guided_last_error, g, gdp_guided_count, gdp_download_guided);
    gdp_guided_destroy(g);
    gdp_ransac_destroy(r);
    gdp_match_destroy(m);
    return out;
}

inline void GaussPyramid_hip::output() {  // :89-104
    int len = length;
    for (int i = 0; i < layer; ++i) {
        for (int j = 0; j < len; ++j) {
            for (int k = 0; k < len; ++k) std::cout << GaussPy[i][0][j][k] << " ";
            std::cout << std::endl;
        }
        for (int k = 0; k < len; ++k) std::cout << "==";
        std::cout << std::endl;
        len /= 2;
    }
}

inline GaussPyramid_hip::~GaussPyramid_hip() {
    if (GaussPy) {
        for (int o = 0; o < layer; ++o) {
            for (int s = 0; s < S + 3; ++s) {
                if (!host_)
                    for (int r = 0; r < (length >> o); ++r) delete[] GaussPy[o][s][r];
                delete[] GaussPy[o][s];
            }
            delete[] GaussPy[o];
        }
        delete[] GaussPy;
    }
    gdp_host_free(host_);
    if (data) {
        for (int i = 0; i < length; ++i) delete[] data[i];
        delete[] data;
    }
    delete[] filter;
    gdp_describe_destroy(describe_);
    gdp_orient_destroy(orient_);
    gdp_destroy(ctx_);
}

#endif  // SIFT_GAUSSDEPYRAMID_HIP_H
