# tests/harness/tensor.mk — ASan + UBSan build of tensor_check (tests/test_tensor_core.py): the
# device-tensor core (csrc/jmh_tensor.h) against integer arithmetic, its formulas and jm_pad_picture of
# host/yuv.c.  Everything is compiled from source with the sanitizers:   make -C tests/harness -f tensor.mk
CC       ?= gcc
ASAN     := _build_asan
HOSTDIR  := ../../h264-jm-commentary_amd/host
CSRC     := ../../h264-jm-commentary_amd/csrc
SANFLAGS := -O2 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all
HDRS     := $(HOSTDIR)/jmhost.h $(CSRC)/jmh_tensor.h $(CSRC)/jmh_rgb.h $(CSRC)/jmh_ingest.h

$(ASAN)/tensor_check: tensor_check.c $(HOSTDIR)/yuv.c $(HDRS)
	mkdir -p $(ASAN)
	$(CC) -std=gnu11 -Wall -Wno-unused-function $(SANFLAGS) -I$(HOSTDIR) -I../../include tensor_check.c $(HOSTDIR)/yuv.c -lm -o $@
