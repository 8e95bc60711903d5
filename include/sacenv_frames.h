/*
 * sacenv_frames.h — episode frames: the frames of one member's kept episode, drawn on the
 * device from the member buffer of sacenv_traces.h.
 *
 * The reference draws the episodes that set a new best as animated GIFs (main.py -r,
 * rendering/boat_env_render.py): per step the track, the path so far, the boat at its heading
 * and a cursor over the time strips. The entry points here draw that picture, palette-indexed
 * (uint8 [F][H][W], SACENV_FRAMES_COLOURS indices), straight from the rows that
 * sacenv_traces_update left on the device. Not drawn: the reference's two wind strips (the
 * rows hold no wind) and its text (that needs a font); the numbers are in the member's header
 * and rows.
 *
 * Conventions as in sacenv_traces.h: device pointers, the descriptor is host memory read
 * during the call, `stream` a hipStream_t, every call only enqueues kernels (stream-ordered,
 * graph-capturable, nothing read back), every error is found on the host before anything is
 * launched; return 0, an SACENV_E_* code or a hipError_t. sacenv.h is untouched:
 * SACENV_ABI_VERSION does not count these.
 *
 * THE PICTURE. All geometry is integer, in sixteenths of a pixel, so a restatement in numpy
 * (tests/frames_oracle.py) gives the same bytes.
 *
 * Layout. A frame is W x H; the top HP = H - S rows are the track panel, the bottom S rows the
 * time strip. Pixel (row r, column c) of the panel has the centre C = (16 c + 8, 16 r + 8).
 *
 * Fixed point. With clamp(v, lo, hi) = !(v >= lo) ? lo : (v > hi ? hi : v), which turns a NaN
 * into lo, and every operation a single f32 one (no contraction):
 *     FX(x) = (int) rint(clamp((x - x0) * scale_x, -1024, 16 W  + 1024))
 *     FY(y) = (int) rint(clamp((y0 - y) * scale_y, -1024, 16 HP + 1024))      (y points up)
 * x0 is the world x of the panel's left edge, y0 the world y of its top edge; the host computes
 * the scales 16 W / (xmax - xmin) and 16 HP / (ymax - ymin) in f64 and rounds them once.
 * Coordinates lie in [-1024, 17408]: a difference of two is at most 18432 < 2^14.2, a dot or
 * cross product of two differences at most 2 * 18432^2 < 2^29.4 (an int32), its square below
 * 2^59 (an int64).
 *
 * Points. Row i of the member (obs f32 x 11 | action | ..) gives
 *     x = obs[0] * goal_line              y = obs[3] * (2 * track_width) - track_width
 *     X_i = FX(x), Y_i = FY(y)
 *     heading_i = (int) rint(clamp(obs[6] * 256, -8388608, 8388608)) & 255
 *     action row  = SR(action)            rudder row = SR(obs[9] * 2 - 1)
 *     SR(a) = (int) rint(clamp((1 - a) * 0.5 * (S - 1), 0, S - 1))      (three f32 products)
 * Row indices count kept rows: of a truncated episode (first_row > 0) row 0 is its first kept row.
 *
 * Path. Segment j (1 <= j <= rows - 1) joins points j - 1 and j. With A, B its ends, d = B - A,
 * p = C - A, t = p.d, a panel pixel is covered by it if
 *     t <= 0:      |p|^2 <= rad^2                (a zero-length segment: the disc of its point)
 *     t >= d.d:    |p - d|^2 <= rad^2
 *     otherwise:   cross(p, d)^2 <= rad^2 * d.d
 * first[pixel] is the smallest j that covers the pixel, INT32_MAX if none does.
 *
 * Frames. Frame f of a call shows step t = min((first_frame + f) * every, rows - 1), rows read
 * on the device from the member's header: frames past the end repeat the last one, and an empty
 * member (rows = 0) gives the background only. A pixel is PATH in frame t iff first[pixel] <= t,
 * so one coverage map serves every frame.
 *
 * Boat. With (ux, uy) = dir[heading_t], f = (ux, -uy) and s = (uy, ux) (f turned a quarter),
 * L = boat_len, G = boat_len >> 1, B = boat_half and >> the arithmetic shift (it floors):
 *     V0 = P_t + ((L f) >> 10)        V1 = P_t + ((-G f - B s) >> 10)        V2 = P_t + ((-G f + B s) >> 10)
 * componentwise. With E(A, B, C) = (B.x - A.x)(C.y - A.y) - (B.y - A.y)(C.x - A.x) a panel pixel is
 * BOAT iff E(V0, V2, C) >= 0, E(V2, V1, C) >= 0 and E(V1, V0, C) >= 0 (all int32).
 *
 * Background. rc = FY(0) >> 4, rt = FY(track_width) >> 4, rb = FY(-track_width) >> 4,
 * cg = FX(goal_line) >> 4. Panel pixel (r, c): OUTSIDE if r < rt or r > rb; else water level
 * min(31, (|r - rc| * 64) / HP) (0 on the centre line); BOUNDARY if r == rt or r == rb; GOAL if
 * c == cg. Priority: BOAT > PATH > GOAL > BOUNDARY > OUTSIDE or water.
 *
 * Strip. Column c shows kept row j(c) = (c * (rows - 1)) / (W - 1) (integer division). Strip
 * pixel (row q = r - HP, column c) is ACTION if j(c) <= t and q lies between the action rows of
 * j(c - 1) and j(c), inclusive (column 0: of j(0) alone); RUDDER the same with the rudder rows.
 * CURSOR is the column (t * (W - 1)) / (rows - 1) (0 with one row), ZERO the row (S - 1) >> 1.
 * Priority: CURSOR > ACTION > RUDDER > ZERO > STRIP. With rows = 0 only ZERO and STRIP.
 *
 * Palette (sacenv/frames.py PALETTE has the colours): indices 0 .. 31 the water levels, then
 * the SACENV_FRAMES_* indices below.
 */
#ifndef SACENV_FRAMES_H
#define SACENV_FRAMES_H

#include "sacenv_traces.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SACENV_FRAMES_VERSION 1
#define SACENV_FRAMES_MIN_DIM 16
#define SACENV_FRAMES_MAX_DIM 1024
#define SACENV_FRAMES_MAX_FRAMES 1048576   /* the largest n_frames of one call */
#define SACENV_FRAMES_MAX_RAD 256
#define SACENV_FRAMES_MAX_BOAT 1024
#define SACENV_FRAMES_CHUNK 128            /* segments a workgroup of the coverage launch stages at a time */
#define SACENV_FRAMES_WATER 32             /* water levels: indices 0 .. 31 */
#define SACENV_FRAMES_OUTSIDE 32
#define SACENV_FRAMES_BOUNDARY 33
#define SACENV_FRAMES_GOAL 34
#define SACENV_FRAMES_PATH 35
#define SACENV_FRAMES_BOAT 36
#define SACENV_FRAMES_STRIP 37
#define SACENV_FRAMES_ZERO 38
#define SACENV_FRAMES_RUDDER 39
#define SACENV_FRAMES_ACTION 40
#define SACENV_FRAMES_CURSOR 41
#define SACENV_FRAMES_COLOURS 42

typedef struct SacenvFrames {
  int32_t width, height;     /* W, H: 16 .. 1024, W a multiple of 4 */
  int32_t strip;             /* S >= 2, H - S >= 8 */
  int32_t members;           /* P and R of the SacenvTraces the member buffer was made with: member m */
  int32_t max_steps;         /*   starts at m * (64 + 64 (R + 1)) */
  int32_t rad;               /* the path's half width, sixteenths of a pixel: 1 .. 256 */
  int32_t boat_len;          /* the boat's nose, sixteenths ahead of its point: 1 .. 1024 */
  int32_t boat_half;         /* its half width at the stern: 1 .. 1024 */
  float x0, y0;              /* world x of the panel's left edge, world y of its top edge */
  float scale_x, scale_y;    /* sixteenths of a pixel per world unit, > 0 */
  float goal_line, track_width;
  int16_t dir[256][2];       /* rint(1024 cos), rint(1024 sin) of 2 pi k / 256, built by the host in f64 */
} SacenvFrames;

/* scratch_bytes: the scratch one render call needs (device, 16-B aligned, opaque: the
 * background's four numbers, 64 B per row -- its fixed-point values and its boat --, 16 B per
 * strip column and the coverage map, 16 + 64 (R + 1) + 16 W + 4 W HP); frame_bytes: W H, one
 * frame of `out`. */
int sacenv_frames_bytes(const SacenvFrames *f, int64_t *scratch_bytes, int64_t *frame_bytes);

/* Draw frames first_frame .. first_frame + n_frames - 1 of member `member` into out
 * (u8 [n_frames][H][W], 4-B aligned), showing every `every`-th step. member_buf is the member
 * buffer of sacenv_traces.h, read only. Three launches: the rows to fixed point, with each row's
 * boat and each strip column's bands; the coverage
 * map (a workgroup per 16 x 16 pixels stages the points through LDS, SACENV_FRAMES_CHUNK
 * segments at a time, and skips a chunk whose bounding box, grown by rad, misses its tile: no
 * byte depends on that); the compose (a thread writes four pixels as one 32-bit store). The
 * call rewrites all of the scratch it reads: a scratch may be shared by calls on one stream.
 *
 * Errors: SACENV_E_NULL (a NULL pointer), SACENV_E_SIZE (width, height, strip, members,
 * max_steps, rad, boat_len or boat_half out of range; member not in 0 .. members - 1; every < 1;
 * n_frames < 1 or > SACENV_FRAMES_MAX_FRAMES), SACENV_E_RANGE (first_frame < 0 or above
 * 2^62; a scale that is not finite and positive, an origin, goal_line or track_width that is
 * not finite; member_buf or scratch not 16-B aligned, out not 4-B aligned). */
int sacenv_frames_render(const SacenvFrames *f, const void *member_buf, int32_t member, int64_t first_frame,
                         int32_t every, int32_t n_frames, void *out, void *scratch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SACENV_FRAMES_H */
