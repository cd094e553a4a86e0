/* ref_map_prelude.h -- forced-include header (-include) of the libref_map builds in oracle/Makefile.
 *
 * TEST INFRASTRUCTURE, ours.  The reference's mapping units reach the FAST5 reader's header through rsig.h, and of all it
 * declares they use one incomplete type (the `hdf5_tools::File *fp` member of ri_sig_file_t) plus the standard headers it
 * happens to pull in.  The builds define that header's include guard (-D__HDF5_TOOLS_HPP), so it is skipped, and this file
 * supplies the two things instead.  Nothing of HDF5 is needed, compiled or linked.
 */
#ifndef RAWDTW_REF_MAP_PRELUDE_H
#define RAWDTW_REF_MAP_PRELUDE_H
#ifdef __cplusplus
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>
namespace hdf5_tools { class File; }
#endif
#endif
