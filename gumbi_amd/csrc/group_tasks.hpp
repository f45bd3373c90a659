// group_tasks.hpp -- the host-side arithmetic of the group averages (group_average.hpp): what is asked of the offsets array, and
// the task list the fused kernels run over.
//
// Group g of a call is the rows [offsets[g], offsets[g + 1]) of its points.  A TASK is a run of at most `chunk` consecutive
// points of one group -- what one workgroup row (blockIdx.y) of group_cov_partial_kernel sums -- so a group of n points has
// ceil(n / chunk) tasks, and every point lies in exactly one.  The list holds (group, first point, count) triples in ascending
// group order and, within a group, ascending first point: the order in which group_cov_finish_kernel adds the partials.
//
// No HIP and no engine types: tools/group_tasks_check.cpp runs this very header on the host.
#pragma once
#include <stdint.h>

#include <vector>

namespace gmb {

constexpr int64_t GROUP_CHUNK = 512;  // points per task (a multiple of the kernels' staged piece)

// What a call asks of offsets[0 .. G]: G >= 1, offsets[0] == 0, strictly increasing (no empty group), offsets[G] == M.
//   0 fine | 1 offsets null or G < 1 | 2 offsets[0] != 0 | 3 offsets[*pos + 1] <= offsets[*pos] (group *pos is empty or runs
//   backwards) | 4 offsets[G] != M
inline int group_check_offsets(const int64_t* offsets, int64_t G, int64_t M, int64_t* pos) {
  if (pos) *pos = -1;
  if (!offsets || G < 1) return 1;
  if (offsets[0] != 0) return 2;
  for (int64_t g = 0; g < G; ++g)
    if (offsets[g + 1] <= offsets[g]) {
      if (pos) *pos = g;
      return 3;
    }
  if (offsets[G] != M) return 4;
  return 0;
}

// tasks of checked offsets (group_check_offsets == 0), chunk >= 1
inline int64_t group_task_count(const int64_t* offsets, int64_t G, int64_t chunk) {
  int64_t n = 0;
  for (int64_t g = 0; g < G; ++g) n += (offsets[g + 1] - offsets[g] + chunk - 1) / chunk;
  return n;
}

// The list for checked offsets: `tasks` takes 3 words per task, (group, first point, count); `first_task`, if given, takes G + 1
// words -- group g's tasks are first_task[g] .. first_task[g + 1] - 1.  Returns the number of tasks.
inline int64_t group_build_tasks(const int64_t* offsets, int64_t G, int64_t chunk, std::vector<int64_t>* tasks,
                                 std::vector<int64_t>* first_task = nullptr) {
  tasks->clear();
  if (first_task) first_task->assign((size_t)G + 1, 0);
  int64_t n = 0;
  for (int64_t g = 0; g < G; ++g) {
    if (first_task) (*first_task)[(size_t)g] = n;
    for (int64_t m0 = offsets[g]; m0 < offsets[g + 1]; m0 += chunk) {
      const int64_t left = offsets[g + 1] - m0;
      tasks->push_back(g);
      tasks->push_back(m0);
      tasks->push_back(left < chunk ? left : chunk);
      ++n;
    }
  }
  if (first_task) (*first_task)[(size_t)G] = n;
  return n;
}

}  // namespace gmb
