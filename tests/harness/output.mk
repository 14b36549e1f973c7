# tests/harness/output.mk — ASan + UBSan build of output_check (tests/test_output_core.py): the
# pulled-picture core (csrc/jmh_output.h), its reference walk into exact-size destinations and its
# argument rules.  Everything is compiled from source with the sanitizers:   make -C tests/harness -f output.mk
CC       ?= gcc
ASAN     := _build_asan
CSRC     := ../../h264-jm-commentary_amd/csrc
SANFLAGS := -O2 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all
HDRS     := $(CSRC)/jmh_output.h $(CSRC)/jmh_tensor.h $(CSRC)/jmh_rgb.h $(CSRC)/jmh_ingest.h

$(ASAN)/output_check: output_check.c $(HDRS)
	mkdir -p $(ASAN)
	$(CC) -std=gnu11 -Wall -Wno-unused-function $(SANFLAGS) output_check.c -o $@
