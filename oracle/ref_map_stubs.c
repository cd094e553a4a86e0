/* ref_map_stubs.c -- the nine symbols the reference's mapping units leave undefined without its file readers.
 *
 * TEST INFRASTRUCTURE, ours.  libref_map{0,1}.so (oracle/Makefile) hold the reference's index, sketch, event, chaining and
 * DTW units but neither its FAST5 reader nor its FASTA reader: ref_map_wrap.cpp hands signal arrays over in memory, so
 * nothing ever calls these.  Should that change, the process stops here instead of running on with a half-made reader.
 * The names have C linkage in the reference's headers; only the names matter to the linker.
 */
#include <stdio.h>
#include <stdlib.h>

#define RAWDTW_STUB(name)                                                                         \
    void name(void)                                                                               \
    {                                                                                             \
        fprintf(stderr, "libref_map: %s is a stub (no file readers in this library)\n", #name);   \
        abort();                                                                                  \
    }

RAWDTW_STUB(find_fast5)
RAWDTW_STUB(open_sig)
RAWDTW_STUB(ri_read_sig)
RAWDTW_STUB(ri_sig_close)
RAWDTW_STUB(ri_seq_to_sig)
RAWDTW_STUB(mm_bseq_open)
RAWDTW_STUB(mm_bseq_close)
RAWDTW_STUB(mm_bseq_eof)
RAWDTW_STUB(mm_bseq_read)
