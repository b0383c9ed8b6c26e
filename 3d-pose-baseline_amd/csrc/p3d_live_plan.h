// p3d_live_plan.h -- which frames of S live OpenPose streams become final in a tick.
// Pure host code, no HIP: a function of the per-slot frame counts and the tick's push and close
// masks, exported as p3d_live_plan (include/p3d.h) so that it can be tested without a GPU.
//
// With smoothing a frame's median window reaches three frames ahead, and whether the frame belongs
// to the clip's last four (which take the four-frame window f-3 .. f) is known only once frame
// f + 4 exists: so frame f is final at n = f + 5 frames, a fixed delay of four pushes.  n = number
// of frames the stream has received:
//   n < 9      nothing (a clip of 2 .. 8 frames is refused; the head windows need frames up to 6)
//   n == 9     frames 0 .. 3 with the head window [f, f+3], frame 4 with the middle window [f-3, f+3]
//   n > 9      frame n - 5, middle window
//   close      n >= 9: frames n-4 .. n-1 with the tail window [f-3, f]; n == 1: the frame unsmoothed;
//              2 <= n <= 8: short (the caller raises); the slot's count returns to 0
// Without smoothing frame n - 1 is final in the tick it arrives and close emits nothing.
#pragma once
#include <stdint.h>

#define P3D_LIVE_KIND_NONE 0     // the frame itself (no smoothing, or a one-frame stream)
#define P3D_LIVE_KIND_HEAD 1     // median of frames f .. f + 3
#define P3D_LIVE_KIND_MIDDLE 2   // median of frames f - 3 .. f + 3
#define P3D_LIVE_KIND_TAIL 3     // median of frames f - 3 .. f
#define P3D_LIVE_SLOT_ROWS 5     // rows a slot can add to one tick
#define P3D_LIVE_DELAY 4         // pushes between a frame and its row, with smoothing
#define P3D_LIVE_MIN_FRAMES 9    // the shortest stream of more than one frame that smoothing takes

// The tick's row table in slot order.  count [S]: frames received so far, updated in place.  push /
// close [S]: non-zero where the slot gets a frame / is closed in this tick (never both).  Out:
// row_off [S + 1] (slot s owns rows row_off[s] .. row_off[s + 1] - 1), row_slot / row_frame /
// row_kind [<= 5 S], push_frame [S] (the stream-local number of the pushed frame, -1: none),
// is_short [S] (closed with 2 .. 8 frames under smoothing).  Returns the number of rows, or -1 - s
// where slot s is both pushed and closed or its count would overflow (nothing is changed then).
inline int64_t live_plan(int64_t S, int smooth, int32_t* count, const uint8_t* push, const uint8_t* close,
                         int64_t* row_off, int32_t* row_slot, int32_t* row_frame, int32_t* row_kind,
                         int32_t* push_frame, int32_t* is_short) {
  for (int64_t s = 0; s < S; ++s)
    if ((push[s] && close[s]) || count[s] < 0 || (push[s] && count[s] == INT32_MAX)) return -1 - s;
  int64_t N = 0;
  const auto emit = [&](int64_t s, int32_t f, int32_t kind) {
    row_slot[N] = (int32_t)s; row_frame[N] = f; row_kind[N] = kind;
    ++N;
  };
  for (int64_t s = 0; s < S; ++s) {
    row_off[s] = N;
    push_frame[s] = -1;
    is_short[s] = 0;
    if (push[s]) {
      push_frame[s] = count[s];
      const int32_t n = ++count[s];
      if (!smooth) emit(s, n - 1, P3D_LIVE_KIND_NONE);
      else if (n == P3D_LIVE_MIN_FRAMES) {
        for (int32_t f = 0; f < 4; ++f) emit(s, f, P3D_LIVE_KIND_HEAD);
        emit(s, 4, P3D_LIVE_KIND_MIDDLE);
      } else if (n > P3D_LIVE_MIN_FRAMES) emit(s, n - 1 - P3D_LIVE_DELAY, P3D_LIVE_KIND_MIDDLE);
    } else if (close[s]) {
      const int32_t n = count[s];
      if (smooth) {
        if (n == 1) emit(s, 0, P3D_LIVE_KIND_NONE);
        else if (n >= P3D_LIVE_MIN_FRAMES)
          for (int32_t f = n - 4; f < n; ++f) emit(s, f, P3D_LIVE_KIND_TAIL);
        else if (n >= 2) is_short[s] = 1;
      }
      count[s] = 0;
    }
  }
  row_off[S] = N;
  return N;
}
