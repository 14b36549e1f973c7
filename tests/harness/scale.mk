# tests/harness/scale.mk — ASan + UBSan build of scale_check (tests/test_scale_core.py): the scaler's
# core (csrc/jmh_scale.h), its reference walk over exact-size buffers and its argument rules.
# Everything is compiled from source with the sanitizers:   make -C tests/harness -f scale.mk
CC       ?= gcc
ASAN     := _build_asan
CSRC     := ../../h264-jm-commentary_amd/csrc
SANFLAGS := -O2 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all
HDRS     := $(CSRC)/jmh_scale.h $(CSRC)/jmh_ingest.h

$(ASAN)/scale_check: scale_check.c $(HDRS)
	mkdir -p $(ASAN)
	$(CC) -std=gnu11 -Wall -Wno-unused-function $(SANFLAGS) scale_check.c -o $@ -lm
