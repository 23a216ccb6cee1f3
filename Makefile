# Build of the MI355X-native DEXTRACTOR codecs.
#   make lib      dextractor_amd/libdexgpu.so   (HIP kernels + C-ABI, gfx950)
#   make cli      dextractor_amd/bin/{dexta,undexta,dexar,undexar,dexqv,undexqv}
#   make oracle   oracle/libdexref.so (+ oracle/_ref/* when /root/reference is present)  [tests only]
HIPCC   ?= /opt/rocm/bin/hipcc
CC      ?= gcc
ARCH    ?= gfx950
CSRC     = dextractor_amd/csrc
BUILD    = build
LIB      = dextractor_amd/libdexgpu.so
EXTRA   ?=
HIPFLAGS = -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Iinclude -I$(CSRC) -Wall -Wno-unused-function $(EXTRA)
CFLAGS   = -O2 -fPIC -Iinclude -Wall -Wextra

# verify/, records/, reads/, digest/, census/, compare/, find/, kmers/, sort/, screen/, place/: device code that came after the evidence set of profiles/ was made (profiles/check.py hashes
# $(CSRC)/*.hip and *.hpp only); units/dx_units.hpp is what four of them share, tiles/dx_tiles.hpp what the tile kernels do (dx_kmers, dx_kmer_runs, dx_kmer_set, dx_screen_spans), find/dx_find_edit.hpp the queries of the two edit-distance files, kmers/dx_kmer_windows.hpp the windows of a chunk and the walk over a unit's chunks (dx_kmers, dx_kmer_codes, dx_kmer_codes_range, dx_kmer_bins, dx_screen, dx_screen_spans, dx_screen_depth, dx_kmer_index, dx_place_seeds), screen/dx_kmer_set.hpp the set of screen/'s files, screen/dx_screen_look.hpp the look-up and the cover mask of screen/'s and place/'s kernels, place/dx_kmer_index.hpp the index of place/'s files, dx_words.h the names of the words of ctx->d_u64
HIP_SRC  = dx_ctx dx_pack2 dx_qv dx_qv_decode dx_synth dx_index dx_qv_walk verify/dx_verify records/dx_qv_records reads/dx_reads reads/dx_lines reads/dx_repack digest/dx_crc census/dx_census compare/dx_diff find/dx_find find/dx_find_edit find/dx_find_span kmers/dx_kmers kmers/dx_kmer_codes kmers/dx_kmer_codes_range kmers/dx_kmer_bins kmers/dx_kmer_runs sort/dx_sort screen/dx_kmer_set screen/dx_screen screen/dx_screen_spans screen/dx_screen_depth place/dx_kmer_index place/dx_place_seeds place/dx_place_vote
HIP_OBJ  = $(HIP_SRC:%=$(BUILD)/%.o)
C_SRC    = dx_host dx_walk_host dx_crew dx_files dx_file_pack2 dx_file_qv dx_file_qv_shard dx_file_check dx_file_u2 dx_file_subset dx_file_extract dx_file_compare dx_file_find dx_file_find_edit dx_file_cut dx_file_kmers dx_file_kmers_wide dx_file_kmers_files dx_file_screen dx_file_screen_spans dx_file_depth dx_file_place dx_select dx_compat
C_OBJ    = $(C_SRC:%=$(BUILD)/%.o)
TOOLS    = dexta undexta dexar undexar dexqv undexqv

all: lib cli

lib: $(LIB)

# every device compile also leaves the kernels' register / LDS / scratch use in $(BUILD)/<file>.res (compiler remarks);
# the library target condenses them into dextractor_amd/kernel_resources.txt, which tests/test_host.py checks:
# some kernels must stay under a register count to share a CU with another kernel
$(BUILD)/%.o: $(CSRC)/%.hip $(CSRC)/dx_internal.hpp $(CSRC)/dx_device.hpp $(CSRC)/dx_layout.h $(CSRC)/dx_walk.h $(CSRC)/dx_host.h $(CSRC)/dx_qv_fast.hpp $(CSRC)/dx_qv_short.hpp $(CSRC)/units/dx_units.hpp $(CSRC)/tiles/dx_tiles.hpp $(CSRC)/find/dx_find_edit.hpp $(CSRC)/kmers/dx_kmer_windows.hpp $(CSRC)/screen/dx_kmer_set.hpp $(CSRC)/screen/dx_screen_look.hpp $(CSRC)/place/dx_kmer_index.hpp $(CSRC)/dx_words.h include/dexgpu.h
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c $< -o $@ 2> $(BUILD)/$*.res; rc=$$?; \
	  grep -v "kernel-resource-usage\|^ *[0-9]* | \|^ *| *^" $(BUILD)/$*.res >&2; exit $$rc

$(BUILD)/%.o: $(CSRC)/%.c $(CSRC)/dx_layout.h $(CSRC)/dx_walk.h $(CSRC)/dx_host.h $(CSRC)/dx_files.h $(CSRC)/dx_crew.h $(CSRC)/dx_env.h include/dexgpu.h include/dexcompat.h
	@mkdir -p $(BUILD)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIB): $(HIP_OBJ) $(C_OBJ)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $^ -Wl,-rpath,/opt/rocm/lib -Wl,-soname,libdexgpu.so -lpthread
	@cat $(HIP_SRC:%=$(BUILD)/%.res) | sed -n 's/.*remark: *//p' | sed 's/ \[-Rpass-analysis=kernel-resource-usage\]//' | \
	  awk '/^Function Name:/ { if (n) print n, v, s, l, o; n = $$3 } /^VGPRs:/ { v = "vgprs=" $$2 } /^ScratchSize/ { s = "scratch=" $$NF } \
	       /^LDS Size/ { l = "lds=" $$NF } /^Occupancy/ { o = "waves_per_simd=" $$NF } END { if (n) print n, v, s, l, o }' \
	  > $(dir $(LIB))kernel_resources$(if $(filter $(LIB),dextractor_amd/libdexgpu.so),,_$(notdir $(basename $(LIB)))).txt

cli: $(LIB) $(TOOLS:%=dextractor_amd/bin/%)

dextractor_amd/bin/%: $(CSRC)/cli/%.c $(CSRC)/cli/cli_common.c $(CSRC)/cli/cli_common.h $(LIB)
	@mkdir -p dextractor_amd/bin
	$(CC) -O2 -Wall -Wextra -Iinclude -I$(CSRC)/cli -o $@ $< $(CSRC)/cli/cli_common.c \
	      -Ldextractor_amd -ldexgpu -Wl,-rpath,'$$ORIGIN/..' -Wl,-rpath,/opt/rocm/lib -lm

oracle:
	$(MAKE) -C oracle all

clean:
	rm -rf $(BUILD) $(LIB) dextractor_amd/bin

# what the library is linked from, for tools/mkvariant.sh: the device files' names, then the host objects
print-objs:
	@echo $(HIP_SRC)
	@echo $(C_OBJ)

.PHONY: all lib cli oracle clean print-objs
